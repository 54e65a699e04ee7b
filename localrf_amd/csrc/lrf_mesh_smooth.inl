// lrf_mesh_smooth.inl -- the faces around each vertex of an indexed triangle mesh (incidence lists), and the three things built
// on them: boundary and non-manifold edge counts, area-weighted vertex normals, and Taubin lambda|mu smoothing (included by
// lrf_render.hip; the scans are lrf_compact.inl's, the host helpers lrf_host.inl's, k_ms_bounds_init is lrf_mesh_simplify.inl's).
// The output bytes are a fixed function of the input: integer counts, integer sums of fixed-point values, and fp64 operations
// that are each rounded on their own (the functions that hold them switch contraction off).  No sort, no floating-point atomics.
//
// A mesh is vertices [Nv,3] fp32 and faces [Nf,3] int32.  A face with an index outside [0, Nv) is never dereferenced: it sets
// bit 0 of the flag word and takes part in nothing.  A face with two equal indices is degenerate: it is counted and takes part
// in nothing.  The other faces are the valid faces.
//
// 1. Incidence lists.  row_start [Nv + 1] and row_faces [3 Nf] int32: row v = row_faces[row_start[v] .. row_start[v + 1]) holds
//    the valid faces with a corner at v.
//      k_sm_zero    deg = 0, the boundary mask = 0, info = 0, E = INT_MIN
//      k_sm_count   one lane per face: atomicAdd(&deg[corner], 1) for its three corners; flag bit 0; info[1] += degenerate faces
//      k_sm_rows    one lane per vertex: the exclusive sum of deg inside its workgroup, the workgroup's total; a row of 2^20
//                   entries or more sets flag bit 1 (the headroom of the int64 sums below)
//      k_points_scan  one workgroup: exclusive bases of the workgroups, info[6] = the number of entries
//      k_sm_starts  row_start[v] += its workgroup's base; row_start[Nv] = entries
//      k_sm_fill    one lane per face: entry row_start[v] + atomicSub(&deg[v], 1) - 1 of each corner v = the face (deg is the
//                   cursor: it ends at 0)
//    THE ORDER INSIDE A ROW DEPENDS ON SCHEDULING.  That is allowed because every consumer below forms integer sums or integer
//    counts over a row, and those do not depend on the order of their terms.  Nothing may read a row in any other way.
// 2. Edges.  For the directed edge (a, b) of valid face f: opp = the directed edges (b, a) among the valid faces, same = the
//    directed edges (a, b) in valid faces other than f.
//      k_sm_edges   one lane per directed edge: it walks the shorter of rows a and b (a tie goes to a; every face that holds the
//                   edge in either direction lies in both rows, so the counts are those of either row) and looks at the three
//                   directed edges of every face there.  opp == 0: a boundary edge, byte stores of 1 at mask[a] and mask[b];
//                   same > 0 or opp > 1: a non-manifold edge.  The ballots' popcounts go to info[2] and info[3], one atomicAdd
//                   per wave each.
// 3. Vertex normals, area-weighted.  Face normal n = (v_b - v_a) x (v_c - v_a) in fp64, every subtract and multiply rounded on
//    its own.  E = the maximum of ilogb(|n_k|) over the non-zero components of all valid faces (int32 atomicMax after a wave
//    maximum: an integer, so no order enters); q_k = llrint(ldexp(n_k, 40 - E)), |q_k| <= 2^41; S_v = the int64 sum of q over
//    row v (exact below 2^20 entries); out = (float)(Nd / sqrt((Nd_x^2 + Nd_y^2) + Nd_z^2)) with Nd = (double)S, or (0, 0, 0)
//    when the length is 0 (counted in info[4]; a vertex in no valid face is one of them).  A face with a coordinate that is
//    not finite contributes 0 and enters E nowhere; a vertex with one sets flag bit 2.
//      k_sm_exponent  one lane per face       k_sm_normals  one lane per vertex (the row sum below)
// 4. One smoothing step with factor f, per vertex v that has n = 2 (row length) > 0 and is not pinned, per axis k:
//    q(x) = llrint(ldexp((double)x - lo_k, s)); S = the int64 sum of q(x_j) over the two other corners j of every face of row
//    v; m = (double)S / (double)n; p = lo_k + ldexp(m, -s); x' = (float)((double)x + f (p - (double)x)), every operation rounded
//    once.  |ldexp(..)| >= 2^41 (or NaN) is clamped and sets flag bit 3: the iteration has diverged.  A pinned vertex and a
//    vertex in no valid face keep their bits.  lo and s come from the host: the per-axis minima of the input (k_sm_bounds: an
//    order-preserving integer image of fp32, -0 read as +0, int32 atomicMin / atomicMax) and 36 - the binary exponent of the
//    largest extent, so the input's q lie in [0, 2^36).
//      k_sm_step    one lane per vertex: a gather from one position buffer into the other, no atomics on positions
// Row sums: a row of up to 64 entries is summed by its vertex's lane.  Longer rows are then summed one after the other by the
// whole wavefront: the lanes stride the row and an int64 shuffle reduction follows.  Integer sums: the same bits either way.
//
// No waiting: every loop is bounded by a row length or by 64, atomics are single instructions that are never retried, and a
// kernel is a fixed sequence: no lane, wave or workgroup waits on another, so nothing here can deadlock under any scheduling.
// Data moves between lanes inside a launch only through the values atomicSub returns (the cursor) and wave shuffles.
namespace lrf {

constexpr int SM_NT = 256;
constexpr int SM_ROW_LIMIT = 1 << 20;
constexpr int SM_LONG_ROW = 64;                                     // longer rows are summed by a wavefront
constexpr double SM_Q_LIMIT = 2199023255552.0;                      // 2^41
constexpr int SM_E_NONE = -0x7fffffff - 1;                          // no non-zero component anywhere
constexpr int SM_S_LIMIT = 256;                                     // |s| of a step: fp32 extents give -93 .. 184
constexpr unsigned long long SM_BAD_FACE = 1, SM_LONG = 2, SM_NOT_FINITE = 4, SM_DIVERGED = 8;
// info [8] int64: flags, degenerate faces, boundary edges, non-manifold edges, zero normals, pinned vertices, entries, 0

struct SmLo { double lo[3]; };

// 0: a valid face, 1: an index outside [0, Nv), 2: degenerate
__device__ __forceinline__ int sm_face(const int* __restrict__ faces, long long f, int Nv, int* a, int* b, int* c) {
  *a = faces[3 * f]; *b = faces[3 * f + 1]; *c = faces[3 * f + 2];
  if (!(in_range(*a, Nv) && in_range(*b, Nv) && in_range(*c, Nv))) return 1;
  return (*a == *b || *b == *c || *a == *c) ? 2 : 0;
}

__global__ __launch_bounds__(SM_NT) void k_sm_zero(int* __restrict__ deg, uint8_t* __restrict__ mask, int Nv,
                                                   unsigned long long* __restrict__ info, int* __restrict__ E) {
  const long long i = (long long)blockIdx.x * SM_NT + threadIdx.x;
  if (i < Nv) { deg[i] = 0; mask[i] = 0; }
  if (i < 8) info[i] = 0ull;
  if (i == 8) *E = SM_E_NONE;
}

__global__ __launch_bounds__(SM_NT) void k_sm_count(const int* __restrict__ faces, int Nf, int Nv, int* deg, unsigned long long* info) {
  const long long f = (long long)blockIdx.x * SM_NT + threadIdx.x;
  int kind = -1, a, b, c;
  if (f < Nf) {
    kind = sm_face(faces, f, Nv, &a, &b, &c);
    if (kind == 0) { atomicAdd(&deg[a], 1); atomicAdd(&deg[b], 1); atomicAdd(&deg[c], 1); }
  }
  wave_or(&info[0], kind == 1, SM_BAD_FACE);
  wave_count(&info[1], kind == 2);
}

__global__ __launch_bounds__(SM_NT) void k_sm_rows(const int* __restrict__ deg, int Nv, int* __restrict__ row_start,
                                                   unsigned* __restrict__ wg, unsigned long long* info) {
  __shared__ unsigned part[SM_NT / 64];
  const long long i = (long long)blockIdx.x * SM_NT + threadIdx.x;
  const unsigned c = i < Nv ? (unsigned)deg[i] : 0u;
  unsigned total;
  const unsigned before = block_scan_excl<SM_NT>(c, part, total);
  if (i < Nv) row_start[i] = (int)before;
  if (threadIdx.x == 0) wg[blockIdx.x] = total;
  wave_or(&info[0], c >= (unsigned)SM_ROW_LIMIT, SM_LONG);
}

__global__ __launch_bounds__(SM_NT) void k_sm_starts(int* __restrict__ row_start, int Nv, const unsigned* __restrict__ wg,
                                                     const unsigned long long* __restrict__ info) {
  const long long i = (long long)blockIdx.x * SM_NT + threadIdx.x;
  if (i < Nv) row_start[i] += (int)wg[i / SM_NT];
  else if (i == Nv) row_start[i] = (int)info[6];
}

__global__ __launch_bounds__(SM_NT) void k_sm_fill(const int* __restrict__ faces, int Nf, int Nv, const int* __restrict__ row_start,
                                                   int* deg, int* __restrict__ row_faces) {
  const long long f = (long long)blockIdx.x * SM_NT + threadIdx.x;
  if (f >= Nf) return;
  int v[3];
  if (sm_face(faces, f, Nv, &v[0], &v[1], &v[2])) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long long at = (long long)row_start[v[k]] + atomicSub(&deg[v[k]], 1) - 1;
    if (at >= 0 && at < 3ll * Nf) row_faces[at] = (int)f;         // always, for the deg that k_sm_count left
  }
}

__device__ __forceinline__ bool sm_has_edge(int g0, int g1, int g2, int a, int b) {
  return (g0 == a && g1 == b) || (g1 == a && g2 == b) || (g2 == a && g0 == b);
}

// item 2's counts of the directed edge (a, b) of valid face f (lrf_mesh_fill.inl's boundary test is this one too)
__device__ __forceinline__ void sm_edge_counts(const int* __restrict__ faces, int Nf, const int* __restrict__ row_start,
                                               const int* __restrict__ row_faces, int f, int a, int b, int* opp_out, int* same_out) {
  const int a0 = row_start[a], na = row_start[a + 1] - a0, b0 = row_start[b], nb = row_start[b + 1] - b0;
  const int at = nb < na ? b0 : a0, n = nb < na ? nb : na;         // the shorter row, a tie goes to a
  int opp = 0, same = 0;
  for (int i = 0; i < n; ++i) {                                     // bounded by the row length
    const int g = row_faces[at + i];
    if (!in_range(g, Nf)) continue;                                    // not a row of k_sm_fill
    const int g0 = faces[3 * (size_t)g], g1 = faces[3 * (size_t)g + 1], g2 = faces[3 * (size_t)g + 2];
    if (sm_has_edge(g0, g1, g2, b, a)) ++opp;
    if (g != f && sm_has_edge(g0, g1, g2, a, b)) ++same;
  }
  *opp_out = opp;
  *same_out = same;
}

__global__ __launch_bounds__(SM_NT) void k_sm_edges(const int* __restrict__ faces, int Nf, int Nv, const int* __restrict__ row_start,
                                                    const int* __restrict__ row_faces, uint8_t* mask, unsigned long long* info) {
  const long long e = (long long)blockIdx.x * SM_NT + threadIdx.x;
  bool boundary = false, nonmanifold = false;
  if (e < 3ll * Nf) {
    const long long f = e / 3;
    const int k = (int)(e - 3 * f);
    int v[3];
    if (sm_face(faces, f, Nv, &v[0], &v[1], &v[2]) == 0) {
      const int a = v[k], b = v[k == 2 ? 0 : k + 1];
      int opp, same;
      sm_edge_counts(faces, Nf, row_start, row_faces, (int)f, a, b, &opp, &same);
      boundary = opp == 0;
      nonmanifold = same > 0 || opp > 1;
      if (boundary) { mask[a] = 1; mask[b] = 1; }                   // plain byte stores of one value
    }
  }
  wave_count(&info[2], boundary);
  wave_count(&info[3], nonmanifold);
}

__global__ __launch_bounds__(SM_NT) void k_sm_pinned(const uint8_t* __restrict__ mask, int Nv, unsigned long long* info) {
  const long long i = (long long)blockIdx.x * SM_NT + threadIdx.x;
  wave_count(&info[5], i < Nv && mask[i] != 0);
}

// the sum over row [begin, begin + n) of vertex v of what add(face, v, acc) adds to acc[3]; EVERY lane of the wave calls it,
// active or not.  Rows of up to SM_LONG_ROW entries: the lane itself; then the longer rows, one after the other, by the wave.
template <class F>
__device__ __forceinline__ void sm_row_sum(const int* __restrict__ row_faces, int v, int begin, int n, bool active, long long* acc,
                                           F add) {
  const int lane = threadIdx.x & 63;
  acc[0] = acc[1] = acc[2] = 0;
  if (active && n <= SM_LONG_ROW)
    for (int i = 0; i < n; ++i) add(row_faces[begin + i], v, acc);
  unsigned long long todo = __ballot(active && n > SM_LONG_ROW);
  while (todo) {                                                    // wave-uniform, at most 64 turns
    const int L = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int vL = __shfl(v, L, 64), bL = __shfl(begin, L, 64), nL = __shfl(n, L, 64);
    long long part[3] = {0, 0, 0};
    for (int i = lane; i < nL; i += 64) add(row_faces[bL + i], vL, part);
#pragma unroll
    for (int k = 0; k < 3; ++k)                                     // wave_sum's order, kept by hand: with the helper k_sm_step zeroes
      for (int off = 32; off > 0; off >>= 1) part[k] += __shfl_xor(part[k], off, 64);   // part with six more moves per turn
    if (lane == L) { acc[0] = part[0]; acc[1] = part[1]; acc[2] = part[2]; }
  }
}

// item 3's face normal -> false when a coordinate is not finite (n = 0 then)
__device__ __forceinline__ bool sm_face_normal(const float* __restrict__ vertices, int a, int b, int c, double* n) {
#pragma clang fp contract(off)
  double pa[3], e1[3], e2[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    pa[k] = (double)vertices[3 * (size_t)a + k];
    const double pb = (double)vertices[3 * (size_t)b + k], pc = (double)vertices[3 * (size_t)c + k];
    ok = ok && is_finite(pa[k]) && is_finite(pb) && is_finite(pc);
    e1[k] = pb - pa[k];
    e2[k] = pc - pa[k];
  }
  if (!ok) { n[0] = n[1] = n[2] = 0.0; return false; }
  const double yz = e1[1] * e2[2], zy = e1[2] * e2[1], zx = e1[2] * e2[0], xz = e1[0] * e2[2], xy = e1[0] * e2[1], yx = e1[1] * e2[0];
  n[0] = yz - zy;
  n[1] = zx - xz;
  n[2] = xy - yx;
  return true;
}

__global__ __launch_bounds__(SM_NT) void k_sm_exponent(const float* __restrict__ vertices, const int* __restrict__ faces, int Nf,
                                                       int Nv, int* E) {
  const long long f = (long long)blockIdx.x * SM_NT + threadIdx.x;
  int e = SM_E_NONE, a, b, c;
  if (f < Nf && sm_face(faces, f, Nv, &a, &b, &c) == 0) {
    double n[3];
    sm_face_normal(vertices, a, b, c, n);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (n[k] == 0.0) continue;
      int x;
      frexp(n[k], &x);                                              // |n_k| = m 2^x with m in [0.5, 1): ilogb = x - 1
      e = max(e, x - 1);
    }
  }
  e = wave_max(e);
  if ((threadIdx.x & 63) == 0 && e != SM_E_NONE) atomicMax(E, e);
}

// item 3's unit normal of the integer sum; false for length 0
__device__ __forceinline__ bool sm_unit(const long long* S, float* out) {
#pragma clang fp contract(off)
  const double x = (double)S[0], y = (double)S[1], z = (double)S[2];
  const double xx = x * x, yy = y * y, zz = z * z;
  const double xy = xx + yy;
  const double len = sqrt(xy + zz);
  if (len == 0.0) { out[0] = out[1] = out[2] = 0.0f; return false; }
  out[0] = (float)(x / len); out[1] = (float)(y / len); out[2] = (float)(z / len);
  return true;
}

__global__ __launch_bounds__(SM_NT) void k_sm_normals(const float* __restrict__ vertices, const int* __restrict__ faces, int Nv,
                                                      int Nf, const int* __restrict__ row_start, const int* __restrict__ row_faces,
                                                      const int* __restrict__ E, float* __restrict__ normals,
                                                      long long* __restrict__ S_out, int* __restrict__ E_out,
                                                      unsigned long long* info) {
  const long long i = (long long)blockIdx.x * SM_NT + threadIdx.x;
  const bool have = i < Nv;
  const int e = *E;
  const int begin = have ? row_start[i] : 0, n = have ? row_start[i + 1] - begin : 0;
  long long S[3];
  sm_row_sum(row_faces, (int)i, begin, n, have && n > 0 && e != SM_E_NONE, S, [&](int g, int, long long* acc) {
    if (!in_range(g, Nf)) return;                                      // not a row of k_sm_fill
    double fn[3];
    sm_face_normal(vertices, faces[3 * (size_t)g], faces[3 * (size_t)g + 1], faces[3 * (size_t)g + 2], fn);
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += llrint(ldexp(fn[k], 40 - e));
  });
  bool zero = false, bad = false;
  if (have) {
    float out[3];
    zero = !sm_unit(S, out);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      bad = bad || !is_finite((double)vertices[3 * i + k]);
      normals[3 * i + k] = out[k];
      if (S_out) S_out[3 * i + k] = S[k];
    }
    if (i == 0 && E_out) *E_out = e;
  }
  wave_count(&info[4], zero);
  wave_or(&info[0], bad, SM_NOT_FINITE);
}

// fp32 -> int32 that orders as the floats do (-0 first made +0)
__device__ __forceinline__ int sm_key(float x) {
  if (x == 0.0f) x = 0.0f;
  const int b = __float_as_int(x);
  return b ^ ((b >> 31) & 0x7fffffff);
}

__global__ __launch_bounds__(SM_NT) void k_sm_bounds(const float* __restrict__ vertices, int Nv, int* out) {
  const long long v = (long long)blockIdx.x * SM_NT + threadIdx.x;
  const bool have = v < Nv;
  float x[3] = {0.0f, 0.0f, 0.0f};
  bool ok = have;
  if (have) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { x[k] = vertices[3 * v + k]; ok = ok && is_finite((double)x[k]); }
  }
  const unsigned long long good = __ballot(ok);
  int lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = wave_min(ok ? sm_key(x[k]) : 0x7fffffff);
    hi[k] = wave_max(ok ? sm_key(x[k]) : -0x7fffffff - 1);
  }
  if ((threadIdx.x & 63) == 0 && good) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { atomicMin(&out[k], lo[k]); atomicMax(&out[3 + k], hi[k]); }
  }
  wave_or(&out[6], have && !ok, 1);
}

// item 4's q -> false when it had to be clamped
__device__ __forceinline__ bool sm_fixed(float x, double lo, int s, long long* q) {
#pragma clang fp contract(off)
  const double d = (double)x - lo;
  const double t = ldexp(d, s);
  if (fabs(t) < SM_Q_LIMIT) { *q = llrint(t); return true; }        // NaN fails
  *q = t > 0.0 ? (long long)SM_Q_LIMIT : t < 0.0 ? -(long long)SM_Q_LIMIT : 0;
  return false;
}

// item 4's new coordinate
__device__ __forceinline__ float sm_moved(float x0, long long S, int n, double lo, int s, double f) {
#pragma clang fp contract(off)
  const double x = (double)x0;
  const double m = (double)S / (double)n;
  const double back = ldexp(m, -s);
  const double p = lo + back;
  const double d = p - x;
  const double fd = f * d;
  return (float)(x + fd);
}

__global__ __launch_bounds__(SM_NT) void k_sm_step(const float* __restrict__ in, float* __restrict__ out, const int* __restrict__ faces,
                                                   int Nv, int Nf, const int* __restrict__ row_start, const int* __restrict__ row_faces,
                                                   const uint8_t* __restrict__ pinned, SmLo lo, int s, double f,
                                                   unsigned long long* info) {
  const long long i = (long long)blockIdx.x * SM_NT + threadIdx.x;
  const bool have = i < Nv;
  const int begin = have ? row_start[i] : 0, n = have ? row_start[i + 1] - begin : 0;
  const bool moves = have && n > 0 && !(pinned && pinned[i]);
  bool diverged = false;
  long long S[3];
  sm_row_sum(row_faces, (int)i, begin, n, moves, S, [&](int g, int v, long long* acc) {
    if (!in_range(g, Nf)) return;                                      // not a row of k_sm_fill
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int j = faces[3 * (size_t)g + t];
      if (j == v || !in_range(j, Nv)) continue;                        // the two other corners
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        long long q;
        if (!sm_fixed(in[3 * (size_t)j + k], lo.lo[k], s, &q)) diverged = true;
        acc[k] += q;
      }
    }
  });
  if (moves) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * i + k] = sm_moved(in[3 * i + k], S[k], 2 * n, lo.lo[k], s, f);
  } else if (have) {
    const unsigned* src = reinterpret_cast<const unsigned*>(in);
    unsigned* dst = reinterpret_cast<unsigned*>(out);
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[3 * i + k] = src[3 * i + k];    // the bits stay
  }
  // not wave_or: as an argument `diverged` becomes a lane mask that the row loop above would have to merge on every entry
  const unsigned long long nd = __ballot(diverged);
  if ((threadIdx.x & 63) == 0 && nd) atomicOr(&info[0], SM_DIVERGED);
}

__global__ __launch_bounds__(SM_NT) void k_sm_copy(const unsigned* __restrict__ in, unsigned* __restrict__ out, long long n) {
  const long long i = (long long)blockIdx.x * SM_NT + threadIdx.x;
  if (i < n) out[i] = in[i];
}

static bool sm_shape(long long Nv, long long Nf) { return mesh_shape(Nv, Nf) && 3 * Nf < (1ll << 31); }
static unsigned sm_blocks(long long n) { return blocks_for(n, SM_NT); }

// the workspace: [E, 8 bytes | row_start Nv + 1 | deg Nv | wg ceil(Nv / 256) | row_faces 3 Nf] int32, [mask Nv] bytes, rounded
// up to 256 (lists: the incidence lists' bytes); lrf_mesh_smooth adds a second position buffer [Nv,3] fp32 behind it (bytes)
struct SmLists { int* E; int* row_start; int* deg; unsigned* wg; int* row_faces; uint8_t* mask; float* tmp; size_t lists, bytes; };
static SmLists sm_lists(void* workspace, long long Nv, long long Nf) {
  Carver c(workspace);
  SmLists p;
  p.E = c.take<int>(2);
  p.row_start = c.take<int>((size_t)Nv + 1);
  p.deg = c.take<int>((size_t)Nv);
  p.wg = c.take<unsigned>(sm_blocks(Nv));
  p.row_faces = c.take<int>(3 * (size_t)Nf);
  p.mask = c.take<uint8_t>((size_t)Nv);
  p.lists = c.at = c.bytes();
  p.tmp = c.take<float>(3 * (size_t)Nv);
  p.bytes = c.bytes();
  return p;
}

// item 1: six launches (four without faces); the mask zeroed is `mask`
static int sm_build(const int* faces, int Nv, int Nf, const SmLists& p, uint8_t* mask, unsigned long long* info, hipStream_t st) {
  LRF_TRY(launch(k_sm_zero, sm_blocks((long long)Nv + 9), SM_NT, st, p.deg, mask, Nv, info, p.E));
  if (Nf) LRF_TRY(launch(k_sm_count, sm_blocks(Nf), SM_NT, st, faces, Nf, Nv, p.deg, info));
  LRF_TRY(launch(k_sm_rows, sm_blocks(Nv), SM_NT, st, p.deg, Nv, p.row_start, p.wg, info));
  LRF_TRY(launch(k_points_scan, 1, PTS_SCAN_NT, st, p.wg, sm_blocks(Nv), reinterpret_cast<long long*>(info + 6)));
  LRF_TRY(launch(k_sm_starts, sm_blocks((long long)Nv + 1), SM_NT, st, p.row_start, Nv, p.wg, info));
  if (Nf) LRF_TRY(launch(k_sm_fill, sm_blocks(Nf), SM_NT, st, faces, Nf, Nv, p.row_start, p.deg, p.row_faces));
  return 0;
}

static int sm_edges(const int* faces, int Nv, int Nf, const SmLists& p, uint8_t* mask, unsigned long long* info, hipStream_t st) {
  if (!Nf) return 0;
  return launch(k_sm_edges, sm_blocks(3ll * Nf), SM_NT, st, faces, Nf, Nv, p.row_start, p.row_faces, mask, info);
}

// the checks every entry point shares -> the refusal's text, or null
static const char* sm_refuse(const void* faces, int64_t Nv, int64_t Nf, const void* info, const void* workspace) {
  if (!sm_shape(Nv, Nf)) return "need 1 <= Nv < 2^31, 0 <= Nf and 3 Nf < 2^31";
  if (!info || !workspace || (Nf && !faces)) return "null argument";
  if (misaligned(3, faces)) return "float and int32 arrays must be 4-byte aligned";
  if (misaligned(7, info, workspace)) return "info and workspace must be 8-byte aligned";
  return nullptr;
}

static int sm_normals(const char* who, const float* vertices, const int32_t* faces, int64_t Nv64, int64_t Nf64, float* normals,
                      int64_t* S_out, int32_t* E_out, int64_t* info64, void* workspace, void* stream) {
  if (const char* why = sm_refuse(faces, Nv64, Nf64, info64, workspace)) return refuse(who, why);
  if (!vertices || !normals) return refuse(who, "null argument");
  if (misaligned(3, vertices, normals, E_out)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, S_out)) return refuse(who, "S must be 8-byte aligned");
  const int Nv = (int)Nv64, Nf = (int)Nf64;
  const SmLists p = sm_lists(workspace, Nv, Nf);
  unsigned long long* info = reinterpret_cast<unsigned long long*>(info64);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(sm_build(faces, Nv, Nf, p, p.mask, info, st));
  if (Nf) LRF_TRY(launch(k_sm_exponent, sm_blocks(Nf), SM_NT, st, vertices, faces, Nf, Nv, p.E));
  return launch(k_sm_normals, sm_blocks(Nv), SM_NT, st, vertices, faces, Nv, Nf, p.row_start, p.row_faces, p.E, normals,
                reinterpret_cast<long long*>(S_out), E_out, info);
}

}  // namespace lrf

extern "C" size_t lrf_mesh_incidence_workspace_bytes(int64_t Nv, int64_t Nf) {
  using namespace lrf;
  return sm_shape(Nv, Nf) ? sm_lists(nullptr, Nv, Nf).lists : 0;
}

extern "C" int lrf_mesh_incidence(const int32_t* faces, int64_t Nv, int64_t Nf, int64_t* info, void* workspace, void* stream) {
  using namespace lrf;
  if (const char* why = sm_refuse(faces, Nv, Nf, info, workspace)) return refuse("lrf_mesh_incidence", why);
  const SmLists p = sm_lists(workspace, Nv, Nf);
  return sm_build(faces, (int)Nv, (int)Nf, p, p.mask, reinterpret_cast<unsigned long long*>(info), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int lrf_mesh_topology(const int32_t* faces, int64_t Nv, int64_t Nf, uint8_t* boundary, int64_t* info, void* workspace,
                                 void* stream) {
  using namespace lrf;
  if (const char* why = sm_refuse(faces, Nv, Nf, info, workspace)) return refuse("lrf_mesh_topology", why);
  if (!boundary) return set_err("lrf_mesh_topology: null argument");
  const SmLists p = sm_lists(workspace, Nv, Nf);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(info);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(sm_build(faces, (int)Nv, (int)Nf, p, boundary, words, st));
  return sm_edges(faces, (int)Nv, (int)Nf, p, boundary, words, st);
}

extern "C" int lrf_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, float* normals,
                                       int64_t* info, void* workspace, void* stream) {
  return lrf::sm_normals("lrf_mesh_vertex_normals", vertices, faces, Nv, Nf, normals, nullptr, nullptr, info, workspace, stream);
}

extern "C" int lrf_debug_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, float* normals,
                                             int64_t* S, int32_t* E, int64_t* info, void* workspace, void* stream) {
  if (!S || !E) return lrf::set_err("lrf_debug_mesh_vertex_normals: null argument");
  return lrf::sm_normals("lrf_debug_mesh_vertex_normals", vertices, faces, Nv, Nf, normals, S, E, info, workspace, stream);
}

extern "C" int lrf_mesh_smooth_bounds(const float* vertices, int64_t Nv, int32_t* out, void* stream) {
  using namespace lrf;
  if (!mesh_shape(Nv, 0)) return set_err("lrf_mesh_smooth_bounds: need 1 <= Nv < 2^31");
  if (!vertices || !out) return set_err("lrf_mesh_smooth_bounds: null argument");
  if (misaligned(3, vertices, out)) return set_err("lrf_mesh_smooth_bounds: float and int32 arrays must be 4-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_ms_bounds_init, 1, 64, st, out));
  return launch(k_sm_bounds, sm_blocks(Nv), SM_NT, st, vertices, Nv, out);
}

extern "C" size_t lrf_mesh_smooth_workspace_bytes(int64_t Nv, int64_t Nf) {
  using namespace lrf;
  return sm_shape(Nv, Nf) ? sm_lists(nullptr, Nv, Nf).bytes : 0;
}

extern "C" int lrf_mesh_smooth(const LrfMeshSmooth* m, float* vertices_out, int64_t* info, void* workspace, void* stream) {
  using namespace lrf;
  if (!m) return set_err("lrf_mesh_smooth: null argument");
  if (const char* why = sm_refuse(m->faces, m->Nv, m->Nf, info, workspace)) return refuse("lrf_mesh_smooth", why);
  if (!m->vertices || !vertices_out) return set_err("lrf_mesh_smooth: null argument");
  if (misaligned(3, m->vertices, vertices_out)) return set_err("lrf_mesh_smooth: float and int32 arrays must be 4-byte aligned");
  if (m->vertices == vertices_out) return set_err("lrf_mesh_smooth: vertices_out must not be the input");
  if (m->iterations < 0 || m->iterations > 1000) return set_err("lrf_mesh_smooth: iterations must lie in [0, 1000]");
  if (!(m->lam > 0.0 && m->lam <= 1.0)) return set_err("lrf_mesh_smooth: need 0 < lam <= 1");
  if (!(m->mu >= -1.0 && m->mu <= 0.0)) return set_err("lrf_mesh_smooth: need -1 <= mu <= 0");
  if (!(is_finite(m->lo[0]) && is_finite(m->lo[1]) && is_finite(m->lo[2]))) return set_err("lrf_mesh_smooth: lo must hold 3 finite values");
  if (m->s < -SM_S_LIMIT || m->s > SM_S_LIMIT) return set_err("lrf_mesh_smooth: s must lie in [-256, 256]");
  const int Nv = (int)m->Nv, Nf = (int)m->Nf;
  const SmLists p = sm_lists(workspace, Nv, Nf);
  unsigned long long* words = reinterpret_cast<unsigned long long*>(info);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(sm_build(m->faces, Nv, Nf, p, p.mask, words, st));
  LRF_TRY(sm_edges(m->faces, Nv, Nf, p, p.mask, words, st));
  const uint8_t* pinned = m->pin_boundary ? p.mask : nullptr;
  if (pinned) LRF_TRY(launch(k_sm_pinned, sm_blocks(Nv), SM_NT, st, pinned, Nv, words));
  const int per = m->mu == 0.0 ? 1 : 2;
  const int steps = m->iterations * per;
  if (!steps)
    return launch(k_sm_copy, sm_blocks(3ll * Nv), SM_NT, st, reinterpret_cast<const unsigned*>(m->vertices),
                  reinterpret_cast<unsigned*>(vertices_out), 3ll * Nv);
  SmLo lo;
  for (int k = 0; k < 3; ++k) lo.lo[k] = m->lo[k];
  const float* in = m->vertices;
  for (int t = 0; t < steps; ++t) {                                 // ping-pong: the last step writes vertices_out
    float* out = ((steps - 1 - t) & 1) ? p.tmp : vertices_out;
    const double f = (per == 2 && (t & 1)) ? m->mu : m->lam;
    LRF_TRY(launch(k_sm_step, sm_blocks(Nv), SM_NT, st, in, out, m->faces, Nv, Nf, p.row_start, p.row_faces, pinned, lo, m->s, f, words));
    in = out;
  }
  return 0;
}
