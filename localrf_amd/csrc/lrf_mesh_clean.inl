// lrf_mesh_clean.inl -- the connected components of an indexed triangle mesh, and the mesh without its small components
// (included by lrf_render.hip; the scan and the keep list are lrf_compact.inl's, the host helpers lrf_host.inl's).  Integers only: no float
// arithmetic touches the data, positions and colours are copied bit for bit.
//
// A mesh is vertices [Nv,3] fp32, rgb8 [Nv,3] uint8 (nullable) and faces [Nf,3] int32.  Two vertices are connected when a face
// holds both; labels[v] is the smallest vertex index of v's component; a vertex that no face holds is a component of its own
// with 0 faces.  The labels are the unique fixed point of the rounds below, so they do not depend on scheduling.
//
// Labelling: min-label hooking with a bounded walk.  parent[v] starts at v (k_cc_init) and only ever decreases, so parent[v]
// <= v with equality exactly at a root, the parent links form a forest, and parent[v] stays inside v's component.  One round
// (lrf_mesh_components_round), with every parent[v] a root when it starts:
//   k_cc_clear    changed = 0
//   k_cc_hook     one lane per face (a, b, c): a face with an index outside [0, Nv) is never dereferenced: it sets bit 1 of
//                 changed and is skipped.  ra, rb, rc = parent[a], parent[b], parent[c]; m = their minimum; for every r of the
//                 three with r > m: old = atomicMin(&parent[r], m) (int32, global memory; one instruction, no retry), and the
//                 face sets bit 0 of changed when old > m.  One lane per wave ORs the wave's bits into changed.
//   k_cc_shorten  one lane per vertex: r = parent[v]; while parent[r] < r: r = parent[r]; parent[v] = r.  A plain store of a
//                 value that is no larger.  Roots are not written during this pass and a lane only ever replaces parent[x] by
//                 an ancestor of x, so every walk ends at the root of its tree, and after the pass every parent[v] is a root.
// A hooking pass that lowers nothing found, for every face, three equal roots (an unequal face has a root r > m with parent[r]
// = r, which its atomicMin lowers unless another lane lowered it first: a change either way).  Then every component has one
// root, and since parent[v] <= v and the root lies in the component, it is the component's smallest index.  Every changing
// round lowers the sum of the parents, so the rounds end; a hook may overwrite another hook's link (atomicMin keeps the
// smaller), which loses nothing: the face that made the lost link sees two roots again in the next round.
// No compare-and-swap loop, no spinning, no lane, wave or workgroup waits on another: every loop is bounded by construction
// (the walk by Nv steps, all others by constants) and a kernel is a fixed sequence, so, like the scan of lrf_points.inl,
// it cannot deadlock under any scheduling.  The host drives the rounds and reads the changed word back after each.
//
// Counting (lrf_mesh_components_count), four launches:
//   k_cc_zero            faces_of = vertices_of = 0, summary = 0
//   k_cc_count_faces     faces_of[labels[a]] += 1 per face (a, b, c) with indices in range; int32 atomicAdd, one per run of
//                        equal labels in a wave (the first active lane's label is added once with its popcount)
//   k_cc_count_vertices  vertices_of[labels[v]] += 1, the same way
//   k_cc_summary         over the roots (labels[v] == v): summary[0] += 1, summary[1] += (faces_of[v] > 0), summary[2] =
//                        max(summary[2], faces_of[v]); 64-bit integer atomics, one per wave.  Integer sums and maxima do not
//                        depend on the order of arrival: the same integers on every run.
//
// Filtering (lrf_mesh_filter), three launches: a component is kept when faces_of[label] >= threshold.
//   k_mesh_filter_mark   one lane per vertex (blockIdx.y = 0) or face (1), 64 consecutive items per wave and step; the wave's
//                        ballot is the keep word of its 64 items (a vertex by its label, a face -- indices in range -- by the
//                        label of its first vertex).  Per word: the kept items before it in its workgroup; per workgroup (16
//                        words): its kept items, and for the vertices its kept roots.
//   k_points_scan        three workgroups: exclusive bases of the vertex and face counts per workgroup, and counts[0..2] =
//                        kept vertices, kept faces, kept components
//   k_mesh_filter_write  a kept item goes to row base + before + popcount(word & lanes below): vertices (and rgb8) are copied,
//                        a face's three indices are replaced by the rows of their vertices, found the same way.  Order is
//                        preserved, so the output bytes are a fixed function of the input.
namespace lrf {

constexpr int CC_NT = 256;
constexpr int MF_NT = 256;
constexpr int MF_WORDS_WAVE = 4;                                    // 64-item steps per wave
constexpr int MF_WORDS_WG = (MF_NT / 64) * MF_WORDS_WAVE;           // keep words per workgroup
constexpr int MF_ITEMS_WG = 64 * MF_WORDS_WG;
static_assert(MF_WORDS_WG == KEEP_GROUP, "a workgroup marks one group of a keep list");

__global__ __launch_bounds__(CC_NT) void k_cc_init(int* __restrict__ parent, int Nv) {
  const long long i = (long long)blockIdx.x * CC_NT + threadIdx.x;
  if (i < Nv) parent[i] = (int)i;
}

__global__ __launch_bounds__(64) void k_cc_clear(int* __restrict__ changed) {
  if (threadIdx.x == 0) *changed = 0;
}

__global__ __launch_bounds__(CC_NT) void k_cc_hook(int* parent, const int* __restrict__ faces, int Nv, int Nf, int* changed) {
  const long long f = (long long)blockIdx.x * CC_NT + threadIdx.x;
  int flag = 0;
  if (f < Nf) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (!(in_range(a, Nv) && in_range(b, Nv) && in_range(c, Nv))) {
      flag = 2;
    } else {
      const int ra = parent[a], rb = parent[b], rc = parent[c];
      if (!(in_range(ra, Nv) && in_range(rb, Nv) && in_range(rc, Nv))) {     // not a parent array of k_cc_init: refused like a bad face
        flag = 2;
      } else {
        const int m = min(ra, min(rb, rc));
        if (ra > m && atomicMin(&parent[ra], m) > m) flag = 1;
        if (rb > m && atomicMin(&parent[rb], m) > m) flag = 1;
        if (rc > m && atomicMin(&parent[rc], m) > m) flag = 1;
      }
    }
  }
  const unsigned long long lowered = __ballot(flag == 1), bad = __ballot(flag == 2);
  const int bits = (lowered ? 1 : 0) | (bad ? 2 : 0);
  if ((threadIdx.x & 63) == 0 && bits) atomicOr(changed, bits);
}

__global__ __launch_bounds__(CC_NT) void k_cc_shorten(int* parent, int Nv) {
  const long long i = (long long)blockIdx.x * CC_NT + threadIdx.x;
  if (i >= Nv) return;
  int r = parent[i];
  if (!in_range(r, Nv)) return;
  // parents strictly decrease along the walk (parent[x] <= x, equal only at a root), so it ends within Nv steps
  for (int step = 0; step < Nv; ++step) {
    const int p = parent[r];
    if ((unsigned)p >= (unsigned)r) break;
    r = p;
  }
  parent[i] = r;
}

__global__ __launch_bounds__(CC_NT) void k_cc_zero(int* __restrict__ faces_of, int* __restrict__ vertices_of, int Nv,
                                                   long long* __restrict__ summary) {
  const long long i = (long long)blockIdx.x * CC_NT + threadIdx.x;
  if (i < Nv) { faces_of[i] = 0; vertices_of[i] = 0; }
  if (i < 3) summary[i] = 0;
}

// of[label] += 1 for every active lane, every lane of the wave calling: the first active lane adds the number of lanes that
// share its label, the others add 1 each
__device__ __forceinline__ void cc_count(int* __restrict__ of, int label, bool active) {
  const int lane = threadIdx.x & 63;
  const unsigned long long act = __ballot(active);
  if (!act) return;                                                 // wave-uniform
  const int lead = __ffsll((long long)act) - 1;
  const int first = __shfl(label, lead, 64);
  const unsigned long long same = __ballot(active && label == first);
  if (lane == lead) atomicAdd(&of[first], (int)__popcll(same));
  else if (active && label != first) atomicAdd(&of[label], 1);
}

__global__ __launch_bounds__(CC_NT) void k_cc_count_faces(const int* __restrict__ labels, const int* __restrict__ faces, int Nv,
                                                          int Nf, int* __restrict__ faces_of) {
  const long long f = (long long)blockIdx.x * CC_NT + threadIdx.x;
  int label = -1;
  if (f < Nf) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (in_range(a, Nv) && in_range(b, Nv) && in_range(c, Nv)) label = labels[a];
  }
  cc_count(faces_of, label, in_range(label, Nv));
}

__global__ __launch_bounds__(CC_NT) void k_cc_count_vertices(const int* __restrict__ labels, int Nv, int* __restrict__ vertices_of) {
  const long long i = (long long)blockIdx.x * CC_NT + threadIdx.x;
  const int label = i < Nv ? labels[i] : -1;
  cc_count(vertices_of, label, in_range(label, Nv));
}

__global__ __launch_bounds__(CC_NT) void k_cc_summary(const int* __restrict__ labels, const int* __restrict__ faces_of, int Nv,
                                                      unsigned long long* __restrict__ summary) {
  const long long i = (long long)blockIdx.x * CC_NT + threadIdx.x;
  const bool root = i < Nv && labels[i] == (int)i;
  int nf = root ? faces_of[i] : 0;
  wave_count(&summary[0], root);
  wave_count(&summary[1], nf > 0);
  nf = wave_max(nf);
  if ((threadIdx.x & 63) == 0 && nf > 0) atomicMax(&summary[2], (unsigned long long)nf);
}

struct MeshFilterArgs {
  const unsigned* vertices; const uint8_t* rgb8; const int* faces; const int* labels; const int* faces_of;
  int Nv, Nf, threshold, n_wg;                                      // n_wg workgroups per array: both arrays padded to it
};

// workspace: bits [2][n_wg MF_WORDS_WG] uint64, pre [2][n_wg MF_WORDS_WG] uint32, wg [3][n_wg] uint32
__global__ __launch_bounds__(MF_NT) void k_mesh_filter_mark(MeshFilterArgs a, unsigned long long* __restrict__ bits,
                                                            unsigned* __restrict__ pre, unsigned* __restrict__ wg) {
  __shared__ unsigned red[MF_NT / 64], red_roots[MF_NT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int which = blockIdx.y;
  const int n = which ? a.Nf : a.Nv;
  const size_t words = (size_t)a.n_wg * MF_WORDS_WG;
  const long long word0 = (long long)blockIdx.x * MF_WORDS_WG + wv * MF_WORDS_WAVE;
  unsigned long long m[MF_WORDS_WAVE];
  unsigned cnt = 0, roots = 0;
#pragma unroll
  for (int k = 0; k < MF_WORDS_WAVE; ++k) {
    const long long i = (word0 + k) * 64 + lane;
    bool keep = false, root = false;
    if (i < n) {
      int v = (int)i;
      if (which) {
        const int fa = a.faces[3 * i], fb = a.faces[3 * i + 1], fc = a.faces[3 * i + 2];
        v = in_range(fa, a.Nv) && in_range(fb, a.Nv) && in_range(fc, a.Nv) ? fa : -1;
      }
      if (v >= 0) {
        const int l = a.labels[v];
        keep = in_range(l, a.Nv) && a.faces_of[l] >= a.threshold;
        root = keep && !which && l == v;
      }
    }
    m[k] = __ballot(keep);
    cnt += (unsigned)__popcll(m[k]);
    roots += (unsigned)__popcll(__ballot(root));
  }
  if (lane == 0) { red[wv] = cnt; red_roots[wv] = roots; }
  __syncthreads();
  unsigned before = 0, total = 0, total_roots = 0;
  for (int w = 0; w < MF_NT / 64; ++w) {
    if (w < wv) before += red[w];
    total += red[w];
    total_roots += red_roots[w];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < MF_WORDS_WAVE; ++k) {                       // every word of the workspace is written
      bits[which * words + word0 + k] = m[k];
      pre[which * words + word0 + k] = before;
      before += (unsigned)__popcll(m[k]);
    }
  }
  if (threadIdx.x == 0) {
    wg[(size_t)which * a.n_wg + blockIdx.x] = total;
    if (!which) wg[(size_t)2 * a.n_wg + blockIdx.x] = total_roots;
  }
}

__global__ __launch_bounds__(MF_NT) void k_mesh_filter_write(MeshFilterArgs a, const unsigned long long* __restrict__ bits,
                                                             const unsigned* __restrict__ pre, const unsigned* __restrict__ wg,
                                                             unsigned* __restrict__ vertices_out, uint8_t* __restrict__ rgb8_out,
                                                             int* __restrict__ faces_out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int which = blockIdx.y;
  const KeepList verts{bits, pre, wg}, mine = verts.pick(which, (size_t)a.n_wg * MF_WORDS_WG);
  const long long word0 = (long long)blockIdx.x * MF_WORDS_WG + wv * MF_WORDS_WAVE;
#pragma unroll
  for (int k = 0; k < MF_WORDS_WAVE; ++k) {
    const size_t i = (size_t)(word0 + k) * 64 + lane;
    if (!mine.kept(i)) continue;                                    // a set bit: the item exists, a face's indices are in range
    const size_t row = mine.rank(i);
    if (!which) {
      for (int c = 0; c < 3; ++c) vertices_out[3 * row + c] = a.vertices[3 * i + c];
      if (rgb8_out)
        for (int c = 0; c < 3; ++c) rgb8_out[3 * row + c] = a.rgb8[3 * i + c];
    } else {
      for (int c = 0; c < 3; ++c) faces_out[3 * row + c] = (int)verts.rank(a.faces[3 * i + c]);
    }
  }
}

static long long mf_workgroups(long long Nv, long long Nf) {
  const long long n = Nv > Nf ? Nv : Nf;
  return (n + MF_ITEMS_WG - 1) / MF_ITEMS_WG;                       // >= 1, < 2^21
}

// the workspace of a filter: the keep lists of the vertices and the faces, each padded to n_wg workgroups, and a third row of
// counts (the kept roots) for the scan
struct MeshFilterWs { int n_wg; unsigned long long* bits; unsigned* pre; unsigned* wg; size_t bytes; };
static MeshFilterWs mf_carve(void* workspace, long long Nv, long long Nf) {
  Carver c(workspace);
  MeshFilterWs w;
  w.n_wg = (int)mf_workgroups(Nv, Nf);
  const size_t words = (size_t)w.n_wg * MF_WORDS_WG;
  w.bits = c.take<unsigned long long>(2 * words);
  w.pre = c.take<unsigned>(2 * words);
  w.wg = c.take<unsigned>(3 * (size_t)w.n_wg);
  w.bytes = c.bytes();
  return w;
}

}  // namespace lrf

extern "C" int lrf_mesh_components_init(int32_t* parent, int64_t Nv, void* stream) {
  using namespace lrf;
  if (!mesh_shape(Nv, 0)) return set_err("lrf_mesh_components_init: need 1 <= Nv < 2^31");
  if (!parent) return set_err("lrf_mesh_components_init: null argument");
  if (misaligned(3, parent)) return set_err("lrf_mesh_components_init: parent must be 4-byte aligned");
  return launch(k_cc_init, blocks_for(Nv, CC_NT), CC_NT, reinterpret_cast<hipStream_t>(stream), parent, Nv);
}

extern "C" int lrf_mesh_components_round(int32_t* parent, const int32_t* faces, int64_t Nv, int64_t Nf, int32_t* changed,
                                         void* stream) {
  using namespace lrf;
  if (!mesh_shape(Nv, Nf)) return set_err("lrf_mesh_components_round: need 1 <= Nv < 2^31 and 0 <= Nf < 2^31");
  if (!parent || !changed || (Nf && !faces)) return set_err("lrf_mesh_components_round: null argument");
  if (misaligned(3, parent, faces, changed)) return set_err("lrf_mesh_components_round: int32 arrays must be 4-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_cc_clear, 1, 64, st, changed));
  if (Nf) LRF_TRY(launch(k_cc_hook, blocks_for(Nf, CC_NT), CC_NT, st, parent, faces, Nv, Nf, changed));
  return launch(k_cc_shorten, blocks_for(Nv, CC_NT), CC_NT, st, parent, Nv);
}

extern "C" int lrf_mesh_components_count(const int32_t* labels, const int32_t* faces, int64_t Nv, int64_t Nf, int32_t* faces_of,
                                         int32_t* vertices_of, int64_t* summary, void* stream) {
  using namespace lrf;
  if (!mesh_shape(Nv, Nf)) return set_err("lrf_mesh_components_count: need 1 <= Nv < 2^31 and 0 <= Nf < 2^31");
  if (!labels || !faces_of || !vertices_of || !summary || (Nf && !faces)) return set_err("lrf_mesh_components_count: null argument");
  if (misaligned(3, labels, faces, faces_of, vertices_of)) return set_err("lrf_mesh_components_count: int32 arrays must be 4-byte aligned");
  if (misaligned(7, summary)) return set_err("lrf_mesh_components_count: summary must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned nbv = blocks_for(Nv, CC_NT);
  LRF_TRY(launch(k_cc_zero, nbv, CC_NT, st, faces_of, vertices_of, Nv, reinterpret_cast<long long*>(summary)));
  if (Nf) LRF_TRY(launch(k_cc_count_faces, blocks_for(Nf, CC_NT), CC_NT, st, labels, faces, Nv, Nf, faces_of));
  LRF_TRY(launch(k_cc_count_vertices, nbv, CC_NT, st, labels, Nv, vertices_of));
  return launch(k_cc_summary, nbv, CC_NT, st, labels, faces_of, Nv, reinterpret_cast<unsigned long long*>(summary));
}

extern "C" size_t lrf_mesh_filter_workspace_bytes(int64_t Nv, int64_t Nf) {
  using namespace lrf;
  return mesh_shape(Nv, Nf) ? mf_carve(nullptr, Nv, Nf).bytes : 0;
}

extern "C" int lrf_mesh_filter(const LrfMeshFilter* m, int32_t threshold, float* vertices_out, uint8_t* rgb8_out,
                               int32_t* faces_out, int64_t* counts, void* workspace, void* stream) {
  using namespace lrf;
  if (!m) return set_err("lrf_mesh_filter: null argument");
  if (!mesh_shape(m->Nv, m->Nf)) return set_err("lrf_mesh_filter: need 1 <= Nv < 2^31 and 0 <= Nf < 2^31");
  if (!m->vertices || !m->labels || !m->faces_of || !vertices_out || !counts || !workspace || (m->Nf && (!m->faces || !faces_out)))
    return set_err("lrf_mesh_filter: null argument");
  if (!m->rgb8 != !rgb8_out) return set_err("lrf_mesh_filter: rgb8 and rgb8_out go together");
  if (threshold < 0) return set_err("lrf_mesh_filter: threshold must be >= 0");
  if (misaligned(3, m->vertices, m->faces, m->labels, m->faces_of, vertices_out, faces_out))
    return set_err("lrf_mesh_filter: float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, counts, workspace)) return set_err("lrf_mesh_filter: counts and workspace must be 8-byte aligned");
  const MeshFilterWs w = mf_carve(workspace, m->Nv, m->Nf);
  MeshFilterArgs a;
  memset(&a, 0, sizeof(a));
  a.vertices = reinterpret_cast<const unsigned*>(m->vertices); a.rgb8 = m->rgb8; a.faces = m->faces;
  a.labels = m->labels; a.faces_of = m->faces_of;
  a.Nv = (int)m->Nv; a.Nf = (int)m->Nf; a.threshold = threshold; a.n_wg = w.n_wg;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_mesh_filter_mark, dim3(w.n_wg, 2), MF_NT, st, a, w.bits, w.pre, w.wg));
  LRF_TRY(launch(k_points_scan, 3, PTS_SCAN_NT, st, w.wg, w.n_wg, reinterpret_cast<long long*>(counts)));
  return launch(k_mesh_filter_write, dim3(w.n_wg, a.Nf ? 2 : 1), MF_NT, st, a, w.bits, w.pre, w.wg,
                reinterpret_cast<unsigned*>(vertices_out), rgb8_out, faces_out);
}
