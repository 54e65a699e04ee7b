// lrf_mesh_fill.inl -- the small holes of an indexed triangle mesh found and closed, each by a fan around one new vertex at the
// mean of its rim (included by lrf_render.hip after lrf_mesh_smooth.inl, whose incidence lists, boundary test, fixed point and
// copy kernel it uses; the scans and the keep list are lrf_compact.inl's, the host helpers lrf_host.inl's).  The output bytes are a
// fixed function of the input: integer counts, integer minima, exact int64 sums of fixed-point values and fp64 operations that are
// each rounded on their own.  No sort, no floating-point atomics, no retried atomics.
//
// A mesh is vertices [Nv,3] fp32, rgb8 [Nv,3] uint8 (nullable) and faces [Nf,3] int32; valid, degenerate and out-of-range faces
// are those of lrf_mesh_smooth.inl: an index outside [0, Nv) is never dereferenced and sets flag bit 0, a degenerate face is
// counted and takes part in nothing.  The directed edge k of face f, (faces[f][k], faces[f][(k + 1) % 3]), has the id 3 f + k.
//
// 1. Boundary edge: a directed edge (a, b) of a valid face with opp == 0 (sm_edge_counts: k_sm_edges' test).  Boundary edges
//    are numbered in the order of their ids.  The kernels below keep the id itself as the edge's number: the ids of the boundary
//    edges order as their numbers 0 .. Nb - 1 do, and every rule below reads the numbers through their order only.
// 2. Simple vertex: exactly one outgoing and exactly one incoming boundary edge (int32 atomicAdd counts; the outgoing edge is
//    recorded with an int32 atomicMin of the id, so the word is the same on every run even where it is not used).  next(e) for
//    e = (a, b) is the boundary edge that leaves b when b is simple, else none.  next is injective where it is defined, so the
//    boundary edges fall into simple cycles and open chains.  A vertex where two holes touch (a bow tie) and a non-manifold rim
//    break their chains: those holes are left alone.
// 3. Fillable loop: a cycle of next of L edges with 3 <= L <= max_edges; its leader is its smallest edge.
// 4. Fill: the fillable loops are ranked by leader.  Loop r adds vertex Nv + r at the mean of the loop's L vertices (the tails
//    of its edges), formed as item 4 of lrf_mesh_smooth.inl forms its means: q = llrint(ldexp((double)x - lo, s)) with lo and s
//    from lrf_mesh_smooth_bounds, S = the int64 sum (L <= 4096 values below 2^41: exact), out = (float)(lo + ldexp((double)S /
//    (double)L, -s)), every operation rounded once.  With rgb8 its colour is, per channel, the integer (2 S + L) / (2 L) of the
//    uint8 sum S: the mean rounded to nearest, a half upwards.  Every edge (a, b) of a fillable loop, in the order of the ids,
//    appends the face (b, a, Nv + r): wound as the face that owns (a, b).  The input's Nv vertices, colours and Nf faces are the
//    output's prefix, copied bit for bit.
//    Hence: every edge of a filled loop has opp == 1 afterwards and the new faces make no edge non-manifold (their edges are
//    the rim's, once each, and those at the new vertex, once per direction); the set of new positions and colours does not
//    depend on the order of the input's faces (their order does); a second fill with the same max_edges adds nothing.
//    A coordinate whose q leaves (-2^41, 2^41) -- lo and s are not those of these vertices -- is clamped and sets flag bit 3.
//
// Kernels, after the six of the incidence lists (sm_build):
//   k_hf_zero     in = out = 0 and first = INT_MAX per vertex, the counters = 0
//   k_hf_edges    one lane per directed edge: the boundary test; a boundary edge (a, b) adds 1 to out[a] and in[b], lowers
//                 first[a] to its id and leaves b in next[e] (else -1); loop_of[e] = -1; the ballots' popcounts count the
//                 boundary and the non-manifold edges, one atomicAdd per wave each
//   k_hf_next     one lane per directed edge: next[e] = first[b] when in[b] == out[b] == 1, else -1
//   k_hf_lead     one lane per directed edge with a next, 64 consecutive edges per wave and step: it walks next and leaves at
//                 the first of (i) an id below its own or none (-1 is below every id): not a leader; (ii) more than max_edges
//                 steps; (iii) its own id: the leader of a loop of the counted length.  The wave's ballot is the keep word.
//   k_points_scan exclusive bases of the leaders per workgroup, and their number
//   k_hf_loops    one lane per leader: it walks its loop once more, writes the loop's rank to loop_of of each member (plain
//                 stores, one writer per edge), forms the int64 position sums and the integer colour sums serially, writes
//                 the new vertex and colour, raises the longest-loop word (int32 atomicMax after a wave maximum) and adds L
//                 to the member count (one atomicAdd per wave)
//   k_hf_members  the keep words of the edges with loop_of >= 0; k_points_scan: their bases
//   k_hf_emit     a member edge writes its face to row Nf + its rank among the members: the order of the ids
//   k_sm_copy, k_hf_bytes   the prefix: vertices and faces as 32-bit words, colours as bytes
//   k_hf_info     one lane: the eight info words; flag bit 4 when a capacity is below Nv + loops or Nf + member edges (every
//                 write above is guarded by its capacity)
// lrf_mesh_holes runs the list up to k_hf_loops without output buffers, and k_hf_info.
//
// Bounds: the walks of k_hf_lead and k_hf_loops take at most max_edges steps, max_edges <= 4096: a condition of the serial
// walk (4096 dependent loads per lane), not a measurement.  A non-leader usually leaves after a few steps, by (i).  Pointer
// doubling for longer loops is out of scope, and so are minimal-area or ear-clipping triangulation, refinement and fairing of
// large patches and loops through vertices that are not simple.  Every other loop is bounded by a row length or a constant.
// Atomics are single instructions that are never retried, and a kernel is a fixed sequence: no lane, wave or workgroup waits on
// another, so nothing here can deadlock under any scheduling.  Everything a lane reads was written by an earlier launch, except
// loop_of, which k_hf_loops only writes.
namespace lrf {

constexpr int HF_NT = 256;
constexpr int HF_WORDS_WAVE = 4;                                    // 64-edge steps per wave
constexpr int HF_WORDS_WG = (HF_NT / 64) * HF_WORDS_WAVE;           // keep words per workgroup
constexpr int HF_ITEMS_WG = 64 * HF_WORDS_WG;
static_assert(HF_WORDS_WG == KEEP_GROUP, "a workgroup marks one group of a keep list");
constexpr int HF_MAX_EDGES = 4096;
constexpr int HF_NO_EDGE = 0x7fffffff;
constexpr unsigned long long HF_OFF_RANGE = 8, HF_CAPACITY = 16;    // flag bits beside SM_BAD_FACE, SM_LONG
// the counters: words 0 .. 7 are the info words of sm_build; then boundary edges, non-manifold edges, leaders, members by the
// scan, members by k_hf_loops, flags
enum { HF_NB = 8, HF_NN, HF_LOOPS, HF_MEMBERS, HF_LOOP_EDGES, HF_FLAGS, HF_WORDS = 16 };
// info [8] int64: flags, degenerate faces, boundary edges, non-manifold edges, fillable loops, edges in fillable loops, the
// longest fillable loop, boundary edges in no fillable loop

__global__ __launch_bounds__(HF_NT) void k_hf_zero(int* __restrict__ in, int* __restrict__ out, int* __restrict__ first, int Nv,
                                                   unsigned long long* __restrict__ words, int* __restrict__ longest) {
  const long long i = (long long)blockIdx.x * HF_NT + threadIdx.x;
  if (i < Nv) { in[i] = 0; out[i] = 0; first[i] = HF_NO_EDGE; }
  if (i >= HF_NB && i < HF_WORDS) words[i] = 0ull;
  if (i == HF_WORDS) *longest = 0;
}

__global__ __launch_bounds__(HF_NT) void k_hf_edges(const int* __restrict__ faces, int Nf, int Nv, const int* __restrict__ row_start,
                                                    const int* __restrict__ row_faces, int* in, int* out, int* first,
                                                    int* __restrict__ next, int* __restrict__ loop_of, unsigned long long* words) {
  const long long e = (long long)blockIdx.x * HF_NT + threadIdx.x;
  bool boundary = false, nonmanifold = false;
  if (e < 3ll * Nf) {
    const long long f = e / 3;
    const int k = (int)(e - 3 * f);
    int v[3], head = -1;
    if (sm_face(faces, f, Nv, &v[0], &v[1], &v[2]) == 0) {
      const int a = v[k], b = v[k == 2 ? 0 : k + 1];
      int opp, same;
      sm_edge_counts(faces, Nf, row_start, row_faces, (int)f, a, b, &opp, &same);
      boundary = opp == 0;
      nonmanifold = same > 0 || opp > 1;
      if (boundary) {
        atomicAdd(&out[a], 1);
        atomicAdd(&in[b], 1);
        atomicMin(&first[a], (int)e);
        head = b;
      }
    }
    next[e] = head;
    loop_of[e] = -1;
  }
  wave_count(&words[HF_NB], boundary);
  wave_count(&words[HF_NN], nonmanifold);
}

__global__ __launch_bounds__(HF_NT) void k_hf_next(int* __restrict__ next, int E3, int Nv, const int* __restrict__ in,
                                                   const int* __restrict__ out, const int* __restrict__ first) {
  const long long e = (long long)blockIdx.x * HF_NT + threadIdx.x;
  if (e >= E3) return;
  const int b = next[e];
  if (!in_range(b, Nv)) return;                                        // -1: not a boundary edge
  const int to = first[b];
  next[e] = (in[b] == 1 && out[b] == 1 && in_range(to, E3)) ? to : -1;
}

// item 3: e leads a fillable loop
__device__ __forceinline__ bool hf_leads(const int* __restrict__ next, int E3, int e, int max_edges) {
  int cur = next[e];
  for (int n = 1; n <= max_edges; ++n) {                            // cur = next^n(e); bounded by max_edges
    if (cur == e) return n >= 3;
    if (cur < e || cur >= E3) return false;                         // a smaller edge leads, or the chain is open (-1)
    cur = next[cur];
  }
  return false;
}

// the mark pass of a keep list over n items: every thread of the workgroup calls; red: HF_NT / 64 words of LDS
template <class F>
__device__ __forceinline__ void hf_mark(long long n, unsigned long long* __restrict__ bits, unsigned* __restrict__ pre,
                                        unsigned* __restrict__ wg, unsigned* red, F keep) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long word0 = (long long)blockIdx.x * HF_WORDS_WG + wv * HF_WORDS_WAVE;
  unsigned long long m[HF_WORDS_WAVE];
  unsigned cnt = 0;
#pragma unroll
  for (int k = 0; k < HF_WORDS_WAVE; ++k) {
    const long long i = (word0 + k) * 64 + lane;
    bool kept = false;
    if (i < n) kept = keep((int)i);
    m[k] = __ballot(kept);
    cnt += (unsigned)__popcll(m[k]);
  }
  if (lane == 0) red[wv] = cnt;
  __syncthreads();
  unsigned before = 0, total = 0;
  for (int w = 0; w < HF_NT / 64; ++w) {
    if (w < wv) before += red[w];
    total += red[w];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < HF_WORDS_WAVE; ++k) {                       // every word of the workspace is written
      bits[word0 + k] = m[k];
      pre[word0 + k] = before;
      before += (unsigned)__popcll(m[k]);
    }
  }
  if (threadIdx.x == 0) wg[blockIdx.x] = total;
}

__global__ __launch_bounds__(HF_NT) void k_hf_lead(const int* __restrict__ next, int E3, int max_edges,
                                                   unsigned long long* __restrict__ bits, unsigned* __restrict__ pre,
                                                   unsigned* __restrict__ wg) {
  __shared__ unsigned red[HF_NT / 64];
  hf_mark(E3, bits, pre, wg, red, [&](int e) { return next[e] >= 0 && hf_leads(next, E3, e, max_edges); });
}

__global__ __launch_bounds__(HF_NT) void k_hf_members(const int* __restrict__ loop_of, int E3, unsigned long long* __restrict__ bits,
                                                      unsigned* __restrict__ pre, unsigned* __restrict__ wg) {
  __shared__ unsigned red[HF_NT / 64];
  hf_mark(E3, bits, pre, wg, red, [&](int e) { return loop_of[e] >= 0; });
}

// item 4's mean of L fixed-point values
__device__ __forceinline__ float hf_mean(long long S, int L, double lo, int s) {
#pragma clang fp contract(off)
  const double m = (double)S / (double)L;
  const double back = ldexp(m, -s);
  return (float)(lo + back);
}

struct HfMesh { const float* vertices; const uint8_t* rgb8; const int* faces; int Nv, Nf, max_edges, s; SmLo lo; };

__global__ __launch_bounds__(HF_NT) void k_hf_loops(HfMesh a, const int* __restrict__ next, KeepList lead, int* __restrict__ loop_of,
                                                    float* __restrict__ vertices_out, uint8_t* __restrict__ rgb8_out, long long cap_v,
                                                    unsigned long long* words, int* longest) {
  const long long e = (long long)blockIdx.x * HF_NT + threadIdx.x;
  const int E3 = 3 * a.Nf;
  int L = 0;
  bool off = false;
  if (e < E3 && lead.kept(e)) {
    const unsigned r = lead.rank(e);
    long long S[3] = {0, 0, 0};
    unsigned C[3] = {0, 0, 0};
    int cur = (int)e;
    for (int n = 0; n < a.max_edges; ++n) {                         // a leader's loop closes within max_edges steps
      loop_of[cur] = (int)r;
      const int tail = a.faces[cur];                                // faces[3 f + k]: in range, the edge is a valid face's
      if (in_range(tail, a.Nv)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          long long q;
          if (!sm_fixed(a.vertices[3 * (size_t)tail + k], a.lo.lo[k], a.s, &q)) off = true;
          S[k] += q;
          if (a.rgb8) C[k] += a.rgb8[3 * (size_t)tail + k];
        }
      }
      ++L;
      cur = next[cur];
      if (cur == (int)e || !in_range(cur, E3)) break;
    }
    const long long row = (long long)a.Nv + r;
    if (vertices_out && row < cap_v) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        vertices_out[3 * row + k] = hf_mean(S[k], L, a.lo.lo[k], a.s);
        if (rgb8_out) rgb8_out[3 * row + k] = (uint8_t)((2u * C[k] + (unsigned)L) / (2u * (unsigned)L));
      }
    }
  }
  const int most = wave_max(L), sum = wave_sum(L);                  // at most 64 x 4096
  if ((threadIdx.x & 63) == 0 && sum) {
    atomicMax(longest, most);
    atomicAdd(&words[HF_LOOP_EDGES], (unsigned long long)sum);
  }
  const unsigned long long bad = __ballot(off);
  if ((threadIdx.x & 63) == 0 && bad) atomicOr(&words[HF_FLAGS], HF_OFF_RANGE);
}

__global__ __launch_bounds__(HF_NT) void k_hf_emit(const int* __restrict__ faces, int Nv, int Nf, const int* __restrict__ loop_of,
                                                   KeepList members, int* __restrict__ faces_out, long long cap_f) {
  const long long e = (long long)blockIdx.x * HF_NT + threadIdx.x;
  if (e >= 3ll * Nf || !members.kept(e)) return;
  const long long row = (long long)Nf + members.rank(e);
  if (row >= cap_f) return;
  const long long f = e / 3;
  const int k = (int)(e - 3 * f);
  faces_out[3 * row] = faces[3 * f + (k == 2 ? 0 : k + 1)];
  faces_out[3 * row + 1] = faces[e];
  faces_out[3 * row + 2] = (int)((long long)Nv + loop_of[e]);
}

__global__ __launch_bounds__(HF_NT) void k_hf_bytes(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * HF_NT + threadIdx.x;
  if (i < n) out[i] = in[i];
}

__global__ __launch_bounds__(64) void k_hf_info(const unsigned long long* __restrict__ words, const int* __restrict__ longest,
                                                long long Nv, long long Nf, long long cap_v, long long cap_f, int emit,
                                                unsigned long long* __restrict__ info) {
  if (threadIdx.x) return;
  const unsigned long long loops = words[HF_LOOPS], members = words[HF_LOOP_EDGES];
  unsigned long long flags = words[0] | words[HF_FLAGS];
  if (emit && (Nv + (long long)loops > cap_v || Nf + (long long)members > cap_f)) flags |= HF_CAPACITY;
  info[0] = flags;
  info[1] = words[1];
  info[2] = words[HF_NB];
  info[3] = words[HF_NN];
  info[4] = loops;
  info[5] = members;
  info[6] = (unsigned long long)*longest;
  info[7] = words[HF_NB] - members;
}

static unsigned hf_blocks(long long n) { return blocks_for(n, HF_NT); }

// the workspace: the incidence lists of lrf_mesh_smooth.inl as one piece, then the counters [16] uint64 and the longest loop, the
// three words per vertex, next and loop_of per directed edge, and the keep lists of the leaders (0) and the members (1)
struct HfWs {
  SmLists lists; unsigned long long* words; int* longest; int* in; int* out; int* first; int* next; int* loop_of;
  int n_wg; unsigned long long* bits; unsigned* pre; unsigned* wg; size_t bytes;
};
static HfWs hf_carve(void* workspace, long long Nv, long long Nf) {
  Carver c(workspace);
  HfWs w;
  w.lists = sm_lists(c.take<char>(sm_lists(nullptr, Nv, Nf).lists), Nv, Nf);
  w.words = c.take<unsigned long long>(HF_WORDS, 256);
  w.longest = c.take<int>(2, 256);
  w.in = c.take<int>((size_t)Nv, 256);
  w.out = c.take<int>((size_t)Nv, 256);
  w.first = c.take<int>((size_t)Nv, 256);
  w.next = c.take<int>(3 * (size_t)Nf, 256);
  w.loop_of = c.take<int>(3 * (size_t)Nf, 256);
  w.n_wg = (int)((3 * Nf + HF_ITEMS_WG - 1) / HF_ITEMS_WG);
  if (w.n_wg < 1) w.n_wg = 1;
  const size_t words = (size_t)w.n_wg * HF_WORDS_WG;
  w.bits = c.take<unsigned long long>(2 * words);
  w.pre = c.take<unsigned>(2 * words);
  w.wg = c.take<unsigned>(2 * (size_t)w.n_wg);
  w.bytes = c.bytes();
  return w;
}

// the checks both entry points share -> the refusal's text, or null
static const char* hf_refuse(const LrfMeshHoles* m, const void* info, const void* workspace) {
  if (!m) return "null argument";
  if (const char* why = sm_refuse(m->faces, m->Nv, m->Nf, info, workspace)) return why;
  if (!m->vertices) return "null argument";
  if (misaligned(3, m->vertices)) return "float and int32 arrays must be 4-byte aligned";
  if (m->max_edges < 3 || m->max_edges > HF_MAX_EDGES) return "max_edges must lie in [3, 4096]";
  if (!(is_finite(m->lo[0]) && is_finite(m->lo[1]) && is_finite(m->lo[2]))) return "lo must hold 3 finite values";
  if (m->s < -SM_S_LIMIT || m->s > SM_S_LIMIT) return "s must lie in [-256, 256]";
  return nullptr;
}

// checked arguments; vertices_out == null: the analysis alone
static int hf_run(const LrfMeshHoles* m, float* vertices_out, uint8_t* rgb8_out, int32_t* faces_out, long long cap_v, long long cap_f,
                  int64_t* info64, void* workspace, void* stream) {
  const int Nv = (int)m->Nv, Nf = (int)m->Nf, E3 = 3 * Nf;
  const HfWs w = hf_carve(workspace, Nv, Nf);
  const size_t words = (size_t)w.n_wg * HF_WORDS_WG;
  const KeepList lead{w.bits, w.pre, w.wg}, members{w.bits + words, w.pre + words, w.wg + w.n_wg};
  unsigned long long* info = reinterpret_cast<unsigned long long*>(info64);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  HfMesh a;
  memset(&a, 0, sizeof(a));
  a.vertices = m->vertices; a.rgb8 = m->rgb8; a.faces = m->faces;
  a.Nv = Nv; a.Nf = Nf; a.max_edges = m->max_edges; a.s = m->s;
  for (int k = 0; k < 3; ++k) a.lo.lo[k] = m->lo[k];
  LRF_TRY(sm_build(m->faces, Nv, Nf, w.lists, w.lists.mask, w.words, st));
  LRF_TRY(launch(k_hf_zero, hf_blocks((long long)Nv + HF_WORDS + 1), HF_NT, st, w.in, w.out, w.first, Nv, w.words, w.longest));
  if (Nf) {
    LRF_TRY(launch(k_hf_edges, hf_blocks(E3), HF_NT, st, m->faces, Nf, Nv, w.lists.row_start, w.lists.row_faces, w.in, w.out, w.first,
                   w.next, w.loop_of, w.words));
    LRF_TRY(launch(k_hf_next, hf_blocks(E3), HF_NT, st, w.next, E3, Nv, w.in, w.out, w.first));
    LRF_TRY(launch(k_hf_lead, w.n_wg, HF_NT, st, w.next, E3, m->max_edges, w.bits, w.pre, w.wg));
    LRF_TRY(launch(k_points_scan, 1, PTS_SCAN_NT, st, w.wg, w.n_wg, reinterpret_cast<long long*>(w.words + HF_LOOPS)));
    LRF_TRY(launch(k_hf_loops, hf_blocks(E3), HF_NT, st, a, w.next, lead, w.loop_of, vertices_out, rgb8_out, cap_v, w.words, w.longest));
  }
  if (vertices_out) {
    if (Nf) {
      LRF_TRY(launch(k_hf_members, w.n_wg, HF_NT, st, w.loop_of, E3, w.bits + words, w.pre + words, w.wg + w.n_wg));
      LRF_TRY(launch(k_points_scan, 1, PTS_SCAN_NT, st, w.wg + w.n_wg, w.n_wg, reinterpret_cast<long long*>(w.words + HF_MEMBERS)));
      LRF_TRY(launch(k_hf_emit, hf_blocks(E3), HF_NT, st, m->faces, Nv, Nf, w.loop_of, members, faces_out, cap_f));
      LRF_TRY(launch(k_sm_copy, sm_blocks(E3), SM_NT, st, reinterpret_cast<const unsigned*>(m->faces), reinterpret_cast<unsigned*>(faces_out),
                     (long long)E3));
    }
    LRF_TRY(launch(k_sm_copy, sm_blocks(3ll * Nv), SM_NT, st, reinterpret_cast<const unsigned*>(m->vertices),
                   reinterpret_cast<unsigned*>(vertices_out), 3ll * Nv));
    if (rgb8_out) LRF_TRY(launch(k_hf_bytes, hf_blocks(3ll * Nv), HF_NT, st, m->rgb8, rgb8_out, 3ll * Nv));
  }
  return launch(k_hf_info, 1, 64, st, w.words, w.longest, (long long)Nv, (long long)Nf, cap_v, cap_f, vertices_out ? 1 : 0, info);
}

}  // namespace lrf

extern "C" size_t lrf_mesh_holes_workspace_bytes(int64_t Nv, int64_t Nf) {
  using namespace lrf;
  return sm_shape(Nv, Nf) ? hf_carve(nullptr, Nv, Nf).bytes : 0;
}

extern "C" int lrf_mesh_holes(const LrfMeshHoles* m, int64_t* info, void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_holes";
  if (const char* why = hf_refuse(m, info, workspace)) return refuse(who, why);
  return hf_run(m, nullptr, nullptr, nullptr, 0, 0, info, workspace, stream);
}

extern "C" int lrf_mesh_fill(const LrfMeshHoles* m, float* vertices_out, uint8_t* rgb8_out, int32_t* faces_out, int64_t cap_v,
                             int64_t cap_f, int64_t* info, void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_fill";
  if (const char* why = hf_refuse(m, info, workspace)) return refuse(who, why);
  if (!vertices_out || (cap_f && !faces_out)) return refuse(who, "null argument");
  if (!m->rgb8 != !rgb8_out) return refuse(who, "rgb8 and rgb8_out go together");
  if (misaligned(3, vertices_out, faces_out)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (cap_v < m->Nv || cap_f < m->Nf || !mesh_shape(cap_v, cap_f)) return refuse(who, "need Nv <= cap_v < 2^31 and Nf <= cap_f < 2^31");
  if (vertices_out == m->vertices || (faces_out && faces_out == m->faces) || (rgb8_out && rgb8_out == m->rgb8))
    return refuse(who, "an output must not be its input");
  return hf_run(m, vertices_out, rgb8_out, faces_out, cap_v, cap_f, info, workspace, stream);
}
