// lrf_cloud.inl -- a point cloud indexed for neighbour queries, and a cloud reduced to one point per cell of a voxel grid: the
// nearest point, the k nearest, the points within a radius, the normals, the voxel grid (included by lrf_render.hip after
// lrf_align.inl, whose al_power_of_two it uses; the grid arithmetic, MdGrid, md_cell, MD_SLACK, md_cells and k_md_bounds_init are
// lrf_mesh_distance.inl's, sm_key and k_sm_copy lrf_mesh_smooth.inl's, the cell of a point, the cluster scan, the integer sums
// and the representative lrf_mesh_simplify.inl's, the scan and the wave-leader counts lrf_compact.inl's, the host helpers
// lrf_host.inl's).  The output bytes are a fixed function of the input: exact minima with an index tie-break, integer counts and
// sums, no float atomics.
//
// Every function below with contraction off; "fp64" means every operation rounded on its own, in the order written.
//   1. points.  A cloud is points [M,3] fp32.  A point with a coordinate that is not finite is skipped and counted
//      (nonfinite_points); it is in no cell, so no query returns it.  Every other point is used, duplicates too.
//   2. the pair (p, q), p the query and q a used point: d_k = (double)p_k - (double)q_k (exact), d2 = (d0 d0 + d1 d1) + d2 d2.
//      This is what item 2 of lrf_mesh_distance.inl yields for a face (i, i, i): every edge is zero, every t is 0, the first
//      segment term stays and no plane term is taken.  fp32 inputs cannot overflow it and d2 is never NaN.  The closest point
//      is q's own three words (the degenerate face's closest point is (float)((double)q_k + 0): the same bits but for a -0,
//      which it turns into +0).
//   3. the grid.  Item 3 of lrf_mesh_distance.inl: box = the per-axis minima and maxima of the used points; cell > 0;
//      dims_k = floor((hi_k - lo_k) / cell) + 1 (the host's arithmetic); cell_k(x) = floor(((double)x - lo_k) / cell), then
//      clamped to [0, dims_k - 1].  A used point lies in exactly ONE cell.  The index holds, in cell order, one 16-byte record
//      per used point: x, y, z and the point's index as the fourth word's bits; a cell's candidates are consecutive 16-byte
//      loads, no list -> point gather.  The order of the records inside a cell is left to an atomic cursor: every consumer
//      below forms an exact minimum with an index tie-break, or an integer count, so no output depends on that order.
//   4. the walk.  Item 4 of lrf_mesh_distance.inl: c = cell(p) and the lane walks the Chebyshev shells r = 0, 1, 2, ... of
//      cells around c, shell cells only, cut to the grid, and evaluates item 2 for every record of every visited cell (each
//      record once: a point has one cell and a cell one shell).  After shell r, with bound = ((double)r cell) (1 - 2^-20), it
//      stops when the deciding d2 < bound bound; or r >= max_k max(c_k, dims_k - 1 - c_k) (the cube covers the grid); or
//      bound > limit (max_distance, or the radius).
//      WHY THE BOUND HOLDS.  Let p' be p clamped onto the grid's box; the clamped index c is p''s cell.  After shell r every
//      record of a cell of the cube [c - r, c + r]^3 has been evaluated.  A point x not met there has its one cell beyond the
//      cube on some axis, so it is at least r cells from p' on that axis: |x - p'| >= r cell.  Clamping onto the box cannot
//      increase a per-axis distance to a point inside the box, and every used point lies inside it, so |x - p| >= |x - p'|
//      on every axis.  The cell expression's rounding moves a cell border by about 1e-10 cells at most; the factor 1 - 2^-20
//      covers it.  So an unvisited point has d2 > bound^2: it can neither win nor tie against a deciding d2 below that, and
//      when bound > limit it lies beyond the limit.
//   5. closest: the lexicographic minimum of (d2, index) over the used points; the deciding d2 is the best.  The hit is dropped
//      when d2 > max_distance max_distance (fp64, one product).  No point in reach: distance +inf, index -1, closest NaN.  A
//      query with a coordinate that is not finite: NaN, -1, NaN.  Otherwise distance = (float)sqrt(d2), an fp64 root.
//   6. knn: the k smallest (d2, index), ascending, k in [1, 8]; the deciding d2 is the k-th best (+inf while fewer than k are
//      held).  Slots without a neighbour, or with d2 > max_distance max_distance: +inf, -1.  A query that is not finite: NaN,
//      -1 in all k slots.  Compiled for K = 1, 2, 4, 8 slots, the smallest K >= k runs; the slots are named registers (every
//      index into them is a constant after unrolling), never a runtime-indexed array.  With self_first >= 0 query i skips the
//      cloud point of index self_first + i -- that record alone: a duplicate of it elsewhere counts, at distance 0.
//   7. radius_count: the used points with d2 <= radius radius (fp64, one product), an int32; nothing decides early, the walk
//      ends by the cube or by bound > radius.  A query that is not finite: -1.  self_first as in item 6.
//   8. the voxel grid.  Items 1-4 of lrf_mesh_simplify.inl over the points: a point's integer cell and 2^-32 fraction (ms_cell),
//      the box of the integer cells, clusters numbered by the ordered scan of the occupied-cell bits, integer atomicAdd sums,
//      ms_position and the rounded mean colour.  A bad point (not finite, or |i| >= 2^30 on an axis) is skipped and counted and
//      has cluster_of = -1.  EVERY occupied cell is emitted, in cluster order, with the number of its points.  The bytes do
//      not depend on the order of the points.
//   9. normals: the eigenvectors of the covariance of a query's neighbourhood, a radius and min_neighbours >= 3 given.
//      NEIGHBOURHOOD.  The used points with d2 <= radius radius, item 7's test, the boundary included; a point equal to the
//      query counts; no self_first.  n is their number.
//      LATTICE.  h, from the host: the smallest power of two with radius / h <= 2^15.  Per neighbour q of the query p:
//      t_k = (long long)rint(((double)q_k - (double)p_k) / h).  fl(d_k d_k) <= d2 <= fl(radius radius) gives |d_k| <= radius
//      (1 + 2^-52), so |t_k| <= 2^15.
//      SUMS, int64 in registers: n, s_k = sum t_k, S_ij = sum t_i t_j for i <= j.
//      NO OVERFLOW.  |t_i t_j| <= 2^30 and a cloud has fewer than 2^31 points: every sum stays below 2^61.  Integer sums are
//      why the result cannot depend on the order in which item 3's cursor left the records of a cell.
//      COVARIANCE, fp64: nd = (double)n, mean_k = (double)s_k / nd, C_ij = (double)S_ij / nd - mean_i mean_j, and trace =
//      (C_00 + C_11) + C_22.  The conversions are exact while a sum is below 2^53 in magnitude: in every neighbourhood of fewer
//      than 2^23 points; beyond that they round to nearest, as any restatement's do.
//      EIGENVECTORS.  A = C, V = the identity, then CL_JACOBI_SWEEPS sweeps of cyclic Jacobi over the pairs (p, q) = (0, 1),
//      (0, 2), (1, 2), r the remaining index.  A pair with a_pq == 0 is skipped.  Otherwise, every operation as written:
//        theta = (a_qq - a_pp) / (2 a_pq);  t = (theta < 0 ? -1 : 1) / (|theta| + sqrt(theta theta + 1))
//        c = 1 / sqrt(t t + 1);  s = t c
//        a_pp = a_pp - t a_pq;  a_qq = a_qq + t a_pq
//        (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq), both from the old pair;  a_pq = 0
//        (v_kp, v_kq) = (c v_kp - s v_kq, s v_kp + c v_kq) for k = 0, 1, 2, both from the old pair
//      Only + - * / and sqrt: their fp64 results are the same bits on the device and in numpy, which acos, cos or atan2 would
//      not give.  An infinite theta (a tiny a_pq) gives t = +-0, c = 1, s = +-0 by IEEE rules: no special case.  The sweep
//      count is a constant: the most any case of tests/cloud_normal_cases.py needs until every off-diagonal entry is 0 or below
//      2^-52 trace (4), plus 2.  A, V and the pairs are named scalars: nothing is indexed at run time.
//      OUTPUTS.  The column: that of V at the smallest of a_00, a_11, a_22, the lowest column among equals.  Its sign: with a
//      viewpoint v (fp32; one for all queries, or one per query), dot = ((v0 - p0) n0 + (v1 - p1) n1) + (v2 - p2) n2 with
//      v_k - p_k = (double)v_k - (double)p_k; dot < 0 flips, dot > 0 does not; without a viewpoint, or with a dot that is 0
//      (or NaN: a viewpoint that is not finite), the component of largest magnitude, the lowest index among equals, is made
//      positive.  normal_k = (float) of the column, flipped or not.  eigenvalues: a_00, a_11, a_22 put in ascending order by
//      three compare-and-swaps ((0,1), (1,2), (0,1); a swap only on <), each (float)(a (h h)).  count = n.
//      DEGENERATE.  n < min_neighbours or trace == 0: normal (0, 0, 0), the eigenvalues as computed (0 with n == 0) and the
//      true count.  A query that is not finite: NaN, NaN, -1.
//      RECORD ORDER.  Without query points the queries are the cloud's own: lane j takes record j, queries its x, y, z and
//      writes row index(j); the rows of the points that are not finite are written by k_cl_normals_rest.  The same bytes as
//      the cloud queried in input order, with the lanes of a wave in the same or neighbouring cells.
//
// Work distribution.  k_cl_bounds, k_cl_fill, k_cl_voxel_bounds: one lane per point.  k_cl_fill runs twice: without records it
// counts (an int32 atomicAdd on the point's one cell), k_points_scan turns the counts into starts, and with the records the
// cursor starts at a copy of the starts and ends as the cell's end.  k_cl_closest, k_cl_knn<K>, k_cl_radius_count, k_cl_normals:
// one lane per query point (k_cl_normals<true>: per record); no atomics, no LDS, no scratch.  k_cl_normals_rest: one lane per
// point.  lrf_cloud_voxel: k_ms_zero, k_ms_mark, k_ms_count_words, k_points_scan, k_ms_accumulate as lrf_mesh_simplify runs them,
// then k_cl_voxel_write, one lane per cluster.
//
// No waiting: every loop is bounded by the grid or by a cell's record count read once; atomics are single instructions that
// are never retried; no lane, wave or workgroup waits on another.
namespace lrf {

constexpr int CL_NT = 256;
constexpr int CL_NONE = 0x7fffffff;

struct ClQuery {
  MdGrid g;
  const unsigned* starts; const unsigned* ends; const float4* records; long long entries;
  const float* points; long long N;
  double limit;                                                     // max_distance, or the radius
  long long self_first;                                             // -1: no query skips a record
};

__device__ __forceinline__ bool cl_load(const float* __restrict__ points, long long i, float (&p)[3]) {
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p[k] = points[3 * i + k];
    finite = finite && (__float_as_uint(p[k]) & 0x7FFFFFFFu) < 0x7F800000u;
  }
  return finite;
}

// out: int64 [8] = nonfinite_points, used points, 0, 0, then six int32 (the keys of lo, of hi), 0 (k_md_bounds_init's layout)
__global__ __launch_bounds__(CL_NT) void k_cl_bounds(const float* __restrict__ points, long long M, unsigned long long* __restrict__ out) {
  const long long i = (long long)blockIdx.x * CL_NT + threadIdx.x;
  float p[3] = {0.0f, 0.0f, 0.0f};
  const bool have = i < M;
  const bool ok = have && cl_load(points, i, p);
  wave_count(&out[0], have && !ok);
  wave_count(&out[1], ok);
  const unsigned long long good = __ballot(ok);
  int* keys = reinterpret_cast<int*>(out + 4);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int lo = wave_min(ok ? sm_key(p[k]) : 0x7fffffff);
    const int hi = wave_max(ok ? sm_key(p[k]) : -0x7fffffff - 1);
    if ((threadIdx.x & 63) == 0 && good) { atomicMin(&keys[k], lo); atomicMax(&keys[3 + k], hi); }
  }
}

// records == null: the count pass (cursor = the counts); else the fill pass (cursor starts at the cell's start)
__global__ __launch_bounds__(CL_NT) void k_cl_fill(const float* __restrict__ points, long long M, MdGrid g, unsigned* __restrict__ cursor,
                                                   float4* __restrict__ records, long long entries) {
  const long long i = (long long)blockIdx.x * CL_NT + threadIdx.x;
  float p[3];
  if (i >= M || !cl_load(points, i, p)) return;
  const int cx = md_cell(p[0], g.lo[0], g.cell, g.dims[0]), cy = md_cell(p[1], g.lo[1], g.cell, g.dims[1]);
  const int cz = md_cell(p[2], g.lo[2], g.cell, g.dims[2]);
  const unsigned at = atomicAdd(&cursor[((long long)cz * g.dims[1] + cy) * g.dims[0] + cx], 1u);
  if (records && (long long)at < entries) records[at] = make_float4(p[0], p[1], p[2], __int_as_float((int)i));
}

// item 5's state
struct ClNearest {
  double d2; int idx; float x[3];
  __device__ __forceinline__ void init() {
    d2 = __longlong_as_double(0x7FF0000000000000ll);
    idx = CL_NONE;
    x[0] = x[1] = x[2] = 0.0f;
  }
  __device__ __forceinline__ void visit(double e, int i, const float4& r) {
    if (e < d2 || (e == d2 && i < idx)) { d2 = e; idx = i; x[0] = r.x; x[1] = r.y; x[2] = r.z; }
  }
  __device__ __forceinline__ double deciding() const { return d2; }
};

// item 6's state: K slots ascending in (d2, index); every subscript below is a constant once the loops are unrolled
template <int K>
struct ClNearestK {
  double d2[K]; int idx[K]; int k;
  __device__ __forceinline__ void init(int k_) {
    k = k_;
#pragma unroll
    for (int j = 0; j < K; ++j) { d2[j] = __longlong_as_double(0x7FF0000000000000ll); idx[j] = CL_NONE; }
  }
  __device__ __forceinline__ void visit(double e, int i, const float4&) {
#pragma unroll
    for (int j = K - 1; j >= 0; --j) {
      if (e < d2[j] || (e == d2[j] && i < idx[j])) {
        if (j + 1 < K) { d2[j + 1] = d2[j]; idx[j + 1] = idx[j]; }
        d2[j] = e; idx[j] = i;
      }
    }
  }
  __device__ __forceinline__ double deciding() const {
    // the slots ascend, so the k-th is the largest of the first k.  Not d2[k - 1] and not a chain of selects on j == k - 1,
    // which the compiler turns back into that runtime index and the slots into scratch
    double e = d2[0];
#pragma unroll
    for (int j = 1; j < K; ++j) e = fmax(e, j < k ? d2[j] : 0.0);
    return e;
  }
};

// item 7's state
struct ClWithin {
  double r2; int n;
  __device__ __forceinline__ void visit(double e, int, const float4&) { n += e <= r2 ? 1 : 0; }
  __device__ __forceinline__ double deciding() const { return __longlong_as_double(0x7FF0000000000000ll); }
};

// item 9's state: the ten integer sums, named so that they stay registers
struct ClMoments {
  double r2, h, p0, p1, p2;
  long long n, s0, s1, s2, s00, s01, s02, s11, s12, s22;
  __device__ __forceinline__ void init(const float (&p)[3], double r2_, double h_) {
    r2 = r2_; h = h_;
    p0 = (double)p[0]; p1 = (double)p[1]; p2 = (double)p[2];
    n = s0 = s1 = s2 = s00 = s01 = s02 = s11 = s12 = s22 = 0;
  }
  __device__ __forceinline__ void visit(double e, int, const float4& r) {
#pragma clang fp contract(off)
    if (!(e <= r2)) return;
    const long long t0 = (long long)rint(((double)r.x - p0) / h), t1 = (long long)rint(((double)r.y - p1) / h);
    const long long t2 = (long long)rint(((double)r.z - p2) / h);
    ++n;
    s0 += t0; s1 += t1; s2 += t2;
    s00 += t0 * t0; s01 += t0 * t1; s02 += t0 * t2;
    s11 += t1 * t1; s12 += t1 * t2; s22 += t2 * t2;
  }
  __device__ __forceinline__ double deciding() const { return __longlong_as_double(0x7FF0000000000000ll); }
};

// the records of cell ci against P
template <class S>
__device__ __forceinline__ void cl_visit(const ClQuery& q, long long ci, const double (&P)[3], int self, S& s) {
#pragma clang fp contract(off)
  const unsigned b = q.starts[ci];
  unsigned e = q.ends[ci];
  if ((long long)e > q.entries) e = (unsigned)q.entries;
  for (unsigned j = b; j < e; ++j) {
    const float4 r = q.records[j];
    const int i = __float_as_int(r.w);
    if (i == self) continue;
    const double d0 = P[0] - (double)r.x, d1 = P[1] - (double)r.y, d2 = P[2] - (double)r.z;
    s.visit((d0 * d0 + d1 * d1) + d2 * d2, i, r);
  }
}

// item 4 for a finite p
template <class S>
__device__ __forceinline__ void cl_walk(const ClQuery& q, const float (&p)[3], int self, S& s) {
#pragma clang fp contract(off)
  const double P[3] = {(double)p[0], (double)p[1], (double)p[2]};
  int c[3], rmax = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = md_cell(p[k], q.g.lo[k], q.g.cell, q.g.dims[k]);
    rmax = max(rmax, max(c[k], q.g.dims[k] - 1 - c[k]));
  }
  const int d0 = q.g.dims[0], d1 = q.g.dims[1], d2 = q.g.dims[2];
  for (int r = 0;; ++r) {
    const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, d2 - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, d1 - 1);
    const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, d0 - 1);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const long long row = ((long long)z * d1 + y) * d0;
        if (z - c[2] == r || c[2] - z == r || y - c[1] == r || c[1] - y == r) {
          for (int x = x0; x <= x1; ++x) cl_visit(q, row + x, P, self, s);
        } else {                                                    // r > 0 here: the two cells of the row that lie on the shell
          if (c[0] - r >= 0) cl_visit(q, row + (c[0] - r), P, self, s);
          if (c[0] + r <= d0 - 1) cl_visit(q, row + (c[0] + r), P, self, s);
        }
      }
    const double bound = ((double)r * q.g.cell) * MD_SLACK;
    if (s.deciding() < bound * bound || r >= rmax || bound > q.limit) break;
  }
}

__device__ __forceinline__ int cl_self(const ClQuery& q, long long i) {
  return q.self_first >= 0 ? (int)(q.self_first + i) : -1;          // a record's index is never negative
}

__global__ __launch_bounds__(CL_NT) void k_cl_closest(ClQuery q, float* __restrict__ distance, int* __restrict__ index,
                                                      float* __restrict__ closest) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * CL_NT + threadIdx.x;
  if (i >= q.N) return;
  const float nan = __uint_as_float(0x7FC00000u);
  float p[3];
  const bool finite = cl_load(q.points, i, p);
  ClNearest s;
  s.init();
  if (finite) cl_walk(q, p, -1, s);
  const bool hit = s.idx != CL_NONE && !(s.d2 > q.limit * q.limit);
  distance[i] = !finite ? nan : (hit ? (float)sqrt(s.d2) : __uint_as_float(0x7F800000u));
  index[i] = hit ? s.idx : -1;
  if (!closest) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) closest[3 * i + k] = hit ? s.x[k] : nan;
}

template <int K>
__global__ __launch_bounds__(CL_NT) void k_cl_knn(ClQuery q, int k, float* __restrict__ distance, int* __restrict__ index) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * CL_NT + threadIdx.x;
  if (i >= q.N) return;
  float p[3];
  const bool finite = cl_load(q.points, i, p);
  ClNearestK<K> s;
  s.init(k);
  if (finite) cl_walk(q, p, cl_self(q, i), s);
  const double reach = q.limit * q.limit;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    if (j >= k) continue;                                           // not a break: the loop must unroll for the slots to stay registers
    const bool hit = s.idx[j] != CL_NONE && !(s.d2[j] > reach);
    distance[i * k + j] = !finite ? __uint_as_float(0x7FC00000u) : (hit ? (float)sqrt(s.d2[j]) : __uint_as_float(0x7F800000u));
    index[i * k + j] = hit ? s.idx[j] : -1;
  }
}

__global__ __launch_bounds__(CL_NT) void k_cl_radius_count(ClQuery q, int* __restrict__ count) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * CL_NT + threadIdx.x;
  if (i >= q.N) return;
  float p[3];
  const bool finite = cl_load(q.points, i, p);
  ClWithin s;
  s.r2 = q.limit * q.limit;
  s.n = 0;
  if (finite) cl_walk(q, p, cl_self(q, i), s);
  count[i] = finite ? s.n : -1;
}

// ------------------------------------------------------------------------------------------------ item 9
constexpr int CL_JACOBI_SWEEPS = 6;                                 // tests/cloud_normal_cases.py: no case needs more than 4

struct ClNormals {
  double h; int min_neighbours; int M;
  const float* view; long long view_stride;                         // null: no viewpoint; stride 0: one for all, 3: per query
  float* normal; float* eigenvalues; int* count;
};

// one rotation of item 9 on the pair (p, q), r the remaining index, every operand a named scalar of the kernel.  A macro, not a
// function over references: with their addresses taken the columns of V are picked through a selected address, out of scratch
#define CL_ROTATE(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                          \
  if (apq != 0.0) {                                                                               \
    const double theta = (aqq - app) / (2.0 * apq);                                               \
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));      \
    const double c = 1.0 / sqrt(t * t + 1.0);                                                     \
    const double s = t * c;                                                                       \
    app = app - t * apq;                                                                          \
    aqq = aqq + t * apq;                                                                          \
    const double x = arp, y = arq;                                                                \
    arp = c * x - s * y;                                                                          \
    arq = s * x + c * y;                                                                          \
    apq = 0.0;                                                                                    \
    const double x0 = v0p, y0 = v0q, x1 = v1p, y1 = v1q, x2 = v2p, y2 = v2q;                      \
    v0p = c * x0 - s * y0; v0q = s * x0 + c * y0;                                                 \
    v1p = c * x1 - s * y1; v1q = s * x1 + c * y1;                                                 \
    v2p = c * x2 - s * y2; v2q = s * x2 + c * y2;                                                 \
  }

// RECORDS: lane j takes record j (q.N = the records) and writes the row of the record's index; else query j of q.points
template <bool RECORDS>
__global__ __launch_bounds__(CL_NT) void k_cl_normals(ClQuery q, ClNormals g) {
#pragma clang fp contract(off)
  const long long j = (long long)blockIdx.x * CL_NT + threadIdx.x;
  if (j >= q.N) return;
  float p[3];
  long long row = j;
  bool finite;
  if (RECORDS) {
    const float4 r = q.records[j];
    p[0] = r.x; p[1] = r.y; p[2] = r.z;
    row = __float_as_int(r.w);
    finite = true;                                                  // only used points have records
    if (!in_range((int)row, g.M)) return;                           // cannot happen in a built index: no row outside the outputs
  } else {
    finite = cl_load(q.points, j, p);
  }
  float* normal = g.normal + 3 * row;
  float* eigen = g.eigenvalues + 3 * row;
  if (!finite) {
    const float nan = __uint_as_float(0x7FC00000u);
    normal[0] = normal[1] = normal[2] = nan;
    eigen[0] = eigen[1] = eigen[2] = nan;
    g.count[row] = -1;
    return;
  }
  ClMoments mo;
  mo.init(p, q.limit * q.limit, g.h);
  cl_walk(q, p, -1, mo);
  double e0 = 0.0, e1 = 0.0, e2 = 0.0, c0 = 0.0, c1 = 0.0, c2 = 0.0;
  bool ok = false;
  if (mo.n > 0) {
    const double nd = (double)mo.n;
    const double m0 = (double)mo.s0 / nd, m1 = (double)mo.s1 / nd, m2 = (double)mo.s2 / nd;
    double a00 = (double)mo.s00 / nd - m0 * m0, a01 = (double)mo.s01 / nd - m0 * m1, a02 = (double)mo.s02 / nd - m0 * m2;
    double a11 = (double)mo.s11 / nd - m1 * m1, a12 = (double)mo.s12 / nd - m1 * m2, a22 = (double)mo.s22 / nd - m2 * m2;
    const double trace = (a00 + a11) + a22;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < CL_JACOBI_SWEEPS; ++sweep) {
      CL_ROTATE(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);             // (0, 1), r = 2
      CL_ROTATE(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);             // (0, 2), r = 1
      CL_ROTATE(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);             // (1, 2), r = 0
    }
    double least = a00;
    c0 = v00; c1 = v10; c2 = v20;
    if (a11 < least) { least = a11; c0 = v01; c1 = v11; c2 = v21; }
    if (a22 < least) { least = a22; c0 = v02; c1 = v12; c2 = v22; }
    e0 = a00; e1 = a11; e2 = a22;
    if (e1 < e0) { const double x = e0; e0 = e1; e1 = x; }
    if (e2 < e1) { const double x = e1; e1 = e2; e2 = x; }
    if (e1 < e0) { const double x = e0; e0 = e1; e1 = x; }
    double dot = 0.0;
    if (g.view) {
      const float* v = g.view + g.view_stride * row;
      const double d0 = (double)v[0] - (double)p[0], d1 = (double)v[1] - (double)p[1], d2 = (double)v[2] - (double)p[2];
      dot = (d0 * c0 + d1 * c1) + d2 * c2;
    }
    bool flip = dot < 0.0;
    if (!(dot < 0.0) && !(dot > 0.0)) {
      double big = c0;
      if (fabs(c1) > fabs(big)) big = c1;
      if (fabs(c2) > fabs(big)) big = c2;
      flip = big < 0.0;
    }
    if (flip) { c0 = -c0; c1 = -c1; c2 = -c2; }
    ok = mo.n >= g.min_neighbours && trace != 0.0;
  }
  const double hh = g.h * g.h;
  normal[0] = ok ? (float)c0 : 0.0f; normal[1] = ok ? (float)c1 : 0.0f; normal[2] = ok ? (float)c2 : 0.0f;
  eigen[0] = (float)(e0 * hh); eigen[1] = (float)(e1 * hh); eigen[2] = (float)(e2 * hh);
  g.count[row] = (int)mo.n;
}
#undef CL_ROTATE

// the rows k_cl_normals<true> does not reach: the cloud points that are not finite
__global__ __launch_bounds__(CL_NT) void k_cl_normals_rest(const float* __restrict__ points, long long M, float* __restrict__ normal,
                                                           float* __restrict__ eigenvalues, int* __restrict__ count) {
  const long long i = (long long)blockIdx.x * CL_NT + threadIdx.x;
  float p[3];
  if (i >= M || cl_load(points, i, p)) return;
  const float nan = __uint_as_float(0x7FC00000u);
#pragma unroll
  for (int k = 0; k < 3; ++k) normal[3 * i + k] = eigenvalues[3 * i + k] = nan;
  count[i] = -1;
}

// ------------------------------------------------------------------------------------------------ item 8
// out: int64 [8] = bad points, used points, 0, 0, then six int32 (lo, hi of the integer cells), 0 (k_md_bounds_init's layout)
__global__ __launch_bounds__(CL_NT) void k_cl_voxel_bounds(const float* __restrict__ points, long long M, MsGrid g,
                                                           unsigned long long* __restrict__ out) {
  const long long v = (long long)blockIdx.x * CL_NT + threadIdx.x;
  int i[3] = {0, 0, 0};
  unsigned long long f[3];
  const bool have = v < M;
  const bool ok = have && ms_cell(points + 3 * v, g.origin, g.cell, i, f);
  wave_count(&out[0], have && !ok);
  wave_count(&out[1], ok);
  const unsigned long long good = __ballot(ok);
  int* box = reinterpret_cast<int*>(out + 4);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int lo = wave_min(ok ? i[k] : 0x7fffffff);
    const int hi = wave_max(ok ? i[k] : -0x7fffffff - 1);
    if ((threadIdx.x & 63) == 0 && good) { atomicMin(&box[k], lo); atomicMax(&box[3 + k], hi); }
  }
}

// one lane per cluster below counts[2], the occupied cells k_points_scan left
__global__ __launch_bounds__(CL_NT) void k_cl_voxel_write(MsGrid g, const unsigned long long* __restrict__ S, const unsigned* __restrict__ nC,
                                                          const int* __restrict__ cell_of, const long long* __restrict__ counts, long long M,
                                                          float* __restrict__ points_out, uint8_t* __restrict__ rgb8_out,
                                                          int* __restrict__ count_out) {
  const long long i = (long long)blockIdx.x * CL_NT + threadIdx.x;
  if (i >= M || i >= counts[2]) return;
  const int lin = cell_of[i];
  const int c[3] = {lin % g.dims[0], (lin / g.dims[0]) % g.dims[1], lin / g.dims[0] / g.dims[1]};
  const unsigned n = nC[4 * i];
  if (n == 0) return;                                               // cannot happen: a cluster is a cell that holds a point
#pragma unroll
  for (int k = 0; k < 3; ++k) points_out[3 * i + k] = ms_position(g.origin[k], g.cell, g.lo[k] + c[k], S[3 * i + k], n);
  if (rgb8_out) {
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb8_out[3 * i + k] = (uint8_t)((2ull * nC[4 * i + 1 + k] + n) / (2ull * n));
  }
  count_out[i] = (int)n;
}

// ------------------------------------------------------------------------------------------------ host side
// the grid's arrays: the scan's total, then a start and an end per cell
struct ClGridWs { long long* total; unsigned* starts; unsigned* ends; size_t bytes; };
static ClGridWs cl_carve(void* grid, long long cells) {
  Carver c(grid);
  ClGridWs w;
  w.total = c.take<long long>(1);
  w.starts = c.take<unsigned>((size_t)cells);
  w.ends = c.take<unsigned>((size_t)cells);
  w.bytes = c.bytes();
  return w;
}

// the voxel grid's workspace, 8-byte words first: [zeroed: flag | cell bits | S | n, C], then the 4-byte arrays
struct ClVoxelWs {
  size_t words_c, n_zero, bytes;
  int* flag; unsigned long long* cell_bits; unsigned long long* S; unsigned* nC; unsigned* pre_c; unsigned* wg_c; int* cell_of;
};
static ClVoxelWs cl_voxel_carve(void* workspace, long long M, long long cells) {
  Carver c(workspace);
  ClVoxelWs w;
  w.words_c = round_up(((size_t)cells + 63) / 64, KEEP_GROUP);
  w.flag = c.take<int>(2);
  w.cell_bits = c.take<unsigned long long>(w.words_c);
  w.S = c.take<unsigned long long>(3 * (size_t)M);
  w.nC = c.take<unsigned>(4 * (size_t)M);
  w.n_zero = c.at / 8;
  w.pre_c = c.take<unsigned>(w.words_c);
  w.wg_c = c.take<unsigned>(w.words_c / KEEP_GROUP);
  w.cell_of = c.take<int>((size_t)M);
  w.bytes = c.bytes();
  return w;
}

// the members every entry point over a cloud index reads; fills g and cells
static int cl_index_args(const char* who, const LrfCloudIndex* a, MdGrid& g, long long& cells) {
  if (!a) return refuse(who, "null argument");
  if (a->M < 1 || a->M >= (1ll << 31)) return refuse(who, "need 1 <= M < 2^31");
  if (a->entries < 0 || a->entries > a->M) return refuse(who, "need 0 <= entries <= M");
  cells = md_cells(a->dims);
  if (!cells) return refuse(who, "need dims >= 1 with fewer than 2^31 cells");
  if (!(a->cell > 0.0) || !is_finite(a->cell) || !is_finite(a->lo[0]) || !is_finite(a->lo[1]) || !is_finite(a->lo[2]))
    return refuse(who, "need a finite cell > 0 and a finite lo");
  if (!a->points || !a->grid) return refuse(who, "null argument");
  if (misaligned(3, a->points)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, a->grid)) return refuse(who, "grid must be 8-byte aligned");
  if (misaligned(15, a->records)) return refuse(who, "records must be 16-byte aligned");
  g.cell = a->cell;
  for (int k = 0; k < 3; ++k) { g.lo[k] = a->lo[k]; g.dims[k] = a->dims[k]; }
  return 0;
}

// what every query shares: the index with its records -> q, without its points
static int cl_query_index(const char* who, const LrfCloudIndex* a, ClQuery& q) {
  memset(&q, 0, sizeof(q));
  long long cells = 0;
  LRF_TRY(cl_index_args(who, a, q.g, cells));
  if (!a->records) return refuse(who, "need the records of a built index");
  const ClGridWs w = cl_carve(a->grid, cells);
  q.starts = w.starts; q.ends = w.ends; q.records = static_cast<const float4*>(a->records); q.entries = a->entries;
  q.self_first = -1;
  return 0;
}

// what the three queries of items 5-7 share: the index, N and the query points -> q
static int cl_query_args(const char* who, const LrfCloudIndex* a, const float* points, int64_t N, ClQuery& q) {
  LRF_TRY(cl_query_index(who, a, q));
  if (N < 1 || N >= (1ll << 31)) return refuse(who, "need 1 <= N < 2^31");
  if (!points) return refuse(who, "null argument");
  if (misaligned(3, points)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  q.points = points; q.N = N;
  return 0;
}

static int cl_self_args(const char* who, const LrfCloudIndex* a, int64_t N, int64_t self_first) {
  if (self_first < -1 || (self_first >= 0 && self_first + N > a->M)) return refuse(who, "need self_first = -1, or 0 <= self_first and self_first + N <= M");
  return 0;
}

}  // namespace lrf

extern "C" int lrf_cloud_index_bounds(const float* points, int64_t M, int64_t* out, void* stream) {
  using namespace lrf;
  const char* who = "lrf_cloud_index_bounds";
  if (M < 1 || M >= (1ll << 31)) return refuse(who, "need 1 <= M < 2^31");
  if (!points || !out) return refuse(who, "null argument");
  if (misaligned(3, points)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, out)) return refuse(who, "out must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  LRF_TRY(launch(k_md_bounds_init, 1, 64, st, o));
  return launch(k_cl_bounds, blocks_for(M, CL_NT), CL_NT, st, points, M, o);
}

extern "C" size_t lrf_cloud_index_workspace_bytes(int64_t cells) {
  return cells >= 1 && cells < (1ll << 31) ? lrf::cl_carve(nullptr, cells).bytes : 0;
}

extern "C" int lrf_cloud_index_build(const LrfCloudIndex* a, void* stream) {
  using namespace lrf;
  const char* who = "lrf_cloud_index_build";
  MdGrid g;
  long long cells = 0;
  LRF_TRY(cl_index_args(who, a, g, cells));
  if (!a->records) return refuse(who, "null argument");
  const ClGridWs w = cl_carve(a->grid, cells);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float4* rec = static_cast<float4*>(a->records);
  LRF_TRY(launch(k_md_zero, blocks_for(cells, MD_NT), MD_NT, st, w.starts, cells));
  LRF_TRY(launch(k_cl_fill, blocks_for(a->M, CL_NT), CL_NT, st, a->points, a->M, g, w.starts, (float4*)nullptr, 0ll));
  LRF_TRY(launch(k_points_scan, 1, PTS_SCAN_NT, st, w.starts, (int)cells, w.total));
  LRF_TRY(launch(k_sm_copy, blocks_for(cells, SM_NT), SM_NT, st, w.starts, w.ends, cells));
  return launch(k_cl_fill, blocks_for(a->M, CL_NT), CL_NT, st, a->points, a->M, g, w.ends, rec, a->entries);
}

extern "C" int lrf_cloud_closest(const LrfCloudIndex* a, const float* points, int64_t N, double max_distance, float* distance,
                                 int32_t* index, float* closest, void* stream) {
  using namespace lrf;
  const char* who = "lrf_cloud_closest";
  ClQuery q;
  LRF_TRY(cl_query_args(who, a, points, N, q));
  if (!(max_distance >= 0.0)) return refuse(who, "max_distance must be >= 0 (infinity allowed)");
  if (!distance || !index) return refuse(who, "null argument");
  if (misaligned(3, distance, index, closest)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  q.limit = max_distance;
  return launch(k_cl_closest, blocks_for(N, CL_NT), CL_NT, reinterpret_cast<hipStream_t>(stream), q, distance, index, closest);
}

extern "C" int lrf_cloud_knn(const LrfCloudIndex* a, const float* points, int64_t N, int32_t k, double max_distance, int64_t self_first,
                             float* distance, int32_t* index, void* stream) {
  using namespace lrf;
  const char* who = "lrf_cloud_knn";
  ClQuery q;
  LRF_TRY(cl_query_args(who, a, points, N, q));
  if (k < 1 || k > LRF_CLOUD_MAX_K) return refuse(who, "k must lie in [1, LRF_CLOUD_MAX_K]");
  if (!(max_distance >= 0.0)) return refuse(who, "max_distance must be >= 0 (infinity allowed)");
  LRF_TRY(cl_self_args(who, a, N, self_first));
  if (!distance || !index) return refuse(who, "null argument");
  if (misaligned(3, distance, index)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  q.limit = max_distance;
  q.self_first = self_first;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const unsigned nb = blocks_for(N, CL_NT);
  if (k == 1) return launch(k_cl_knn<1>, nb, CL_NT, st, q, k, distance, index);
  if (k == 2) return launch(k_cl_knn<2>, nb, CL_NT, st, q, k, distance, index);
  if (k <= 4) return launch(k_cl_knn<4>, nb, CL_NT, st, q, k, distance, index);
  return launch(k_cl_knn<8>, nb, CL_NT, st, q, k, distance, index);
}

extern "C" int lrf_cloud_radius_count(const LrfCloudIndex* a, const float* points, int64_t N, double radius, int64_t self_first,
                                      int32_t* count, void* stream) {
  using namespace lrf;
  const char* who = "lrf_cloud_radius_count";
  ClQuery q;
  LRF_TRY(cl_query_args(who, a, points, N, q));
  if (!(radius >= 0.0) || !is_finite(radius)) return refuse(who, "radius must be finite and >= 0");
  LRF_TRY(cl_self_args(who, a, N, self_first));
  if (!count) return refuse(who, "null argument");
  if (misaligned(3, count)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  q.limit = radius;
  q.self_first = self_first;
  return launch(k_cl_radius_count, blocks_for(N, CL_NT), CL_NT, reinterpret_cast<hipStream_t>(stream), q, count);
}

extern "C" int lrf_cloud_normals(const LrfCloudIndex* a, const float* points, int64_t N, double radius, double h, int32_t min_neighbours,
                                 const float* viewpoints, int64_t viewpoint_stride, float* normal, float* eigenvalues, int32_t* count,
                                 void* stream) {
  using namespace lrf;
  const char* who = "lrf_cloud_normals";
  ClQuery q;
  LRF_TRY(cl_query_index(who, a, q));
  if (N < 0 || N >= (1ll << 31)) return refuse(who, "need 0 <= N < 2^31");
  if (!(radius > 0.0) || !is_finite(radius)) return refuse(who, "radius must be finite and > 0");
  if (!al_power_of_two(h)) return refuse(who, "h must be a positive power of two");
  if (!(radius / h <= 32768.0) || radius / (0.5 * h) <= 32768.0)
    return refuse(who, "h must be the smallest power of two with radius / h <= 2^15");
  if (min_neighbours < 3) return refuse(who, "min_neighbours must be >= 3");
  if (viewpoint_stride != 0 && viewpoint_stride != 3)
    return refuse(who, "viewpoint_stride must be 0 (one viewpoint) or 3 (one per query)");
  if (!normal || !eigenvalues || !count) return refuse(who, "null argument");
  if (misaligned(3, points, viewpoints, normal, eigenvalues, count)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (!points && N != a->M) return refuse(who, "without points the queries are the cloud's own: need N == M");
  if (!N) return 0;
  ClNormals g;
  memset(&g, 0, sizeof(g));
  g.h = h; g.min_neighbours = min_neighbours; g.M = (int)(points ? N : a->M);
  g.view = viewpoints; g.view_stride = viewpoint_stride;
  g.normal = normal; g.eigenvalues = eigenvalues; g.count = count;
  q.limit = radius;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (points) {
    q.points = points; q.N = N;
    return launch(k_cl_normals<false>, blocks_for(N, CL_NT), CL_NT, st, q, g);
  }
  LRF_TRY(launch(k_cl_normals_rest, blocks_for(a->M, CL_NT), CL_NT, st, a->points, (long long)a->M, normal, eigenvalues, count));
  q.N = a->entries;
  if (!q.N) return 0;
  return launch(k_cl_normals<true>, blocks_for(q.N, CL_NT), CL_NT, st, q, g);
}

extern "C" int lrf_cloud_voxel_bounds(const float* points, int64_t M, const double* origin, double cell, int64_t* out, void* stream) {
  using namespace lrf;
  const char* who = "lrf_cloud_voxel_bounds";
  if (M < 1 || M >= (1ll << 31)) return refuse(who, "need 1 <= M < 2^31");
  if (!points || !origin || !out) return refuse(who, "null argument");
  if (!(is_finite(origin[0]) && is_finite(origin[1]) && is_finite(origin[2]))) return refuse(who, "origin must hold 3 finite values");
  if (!(cell > 0.0 && is_finite(cell))) return refuse(who, "cell must be finite and > 0");
  if (misaligned(3, points)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, out)) return refuse(who, "out must be 8-byte aligned");
  MsGrid g;
  memset(&g, 0, sizeof(g));
  for (int k = 0; k < 3; ++k) g.origin[k] = origin[k];
  g.cell = cell;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  LRF_TRY(launch(k_md_bounds_init, 1, 64, st, o));
  return launch(k_cl_voxel_bounds, blocks_for(M, CL_NT), CL_NT, st, points, M, g, o);
}

extern "C" size_t lrf_cloud_voxel_workspace_bytes(int64_t M, int64_t cells) {
  using namespace lrf;
  return M >= 1 && M < (1ll << 31) && cells >= 1 && cells < (1ll << 31) ? cl_voxel_carve(nullptr, M, cells).bytes : 0;
}

extern "C" int lrf_cloud_voxel(const LrfCloudVoxel* a, float* points_out, uint8_t* rgb8_out, int32_t* count_out, int32_t* cluster_of,
                               int64_t* counts, void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_cloud_voxel";
  if (!a) return refuse(who, "null argument");
  if (a->M < 1 || a->M >= (1ll << 31)) return refuse(who, "need 1 <= M < 2^31");
  if (!a->points || !points_out || !count_out || !cluster_of || !counts || !workspace) return refuse(who, "null argument");
  if (!a->rgb8 != !rgb8_out) return refuse(who, "rgb8 and rgb8_out go together");
  const long long cells = md_cells(a->dims);
  if (!cells) return refuse(who, "need dims >= 1 with fewer than 2^31 cells");
  for (int k = 0; k < 3; ++k)
    if (a->lo[k] <= -(1 << 30) || (long long)a->lo[k] + a->dims[k] > (1 << 30)) return refuse(who, "the box must lie inside (-2^30, 2^30)");
  if (!(is_finite(a->origin[0]) && is_finite(a->origin[1]) && is_finite(a->origin[2]))) return refuse(who, "origin must hold 3 finite values");
  if (!(a->cell > 0.0 && is_finite(a->cell))) return refuse(who, "cell must be finite and > 0");
  if (misaligned(3, a->points, points_out, count_out, cluster_of)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, counts, workspace)) return refuse(who, "counts and workspace must be 8-byte aligned");
  const int M = (int)a->M;
  const ClVoxelWs w = cl_voxel_carve(workspace, a->M, cells);
  MsGrid g;
  memset(&g, 0, sizeof(g));
  for (int k = 0; k < 3; ++k) { g.origin[k] = a->origin[k]; g.lo[k] = a->lo[k]; g.dims[k] = a->dims[k]; }
  g.cell = a->cell;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  long long* cnt = reinterpret_cast<long long*>(counts);
  const size_t zero_blocks = (w.n_zero + MS_NT - 1) / MS_NT;
  const unsigned nbv = blocks_for(M, MS_NT);
  LRF_TRY(launch(k_ms_zero, (unsigned)(zero_blocks < MS_ZERO_BLOCKS ? zero_blocks : MS_ZERO_BLOCKS), MS_NT, st,
                 static_cast<unsigned long long*>(workspace), w.n_zero, static_cast<unsigned long long*>(nullptr), (size_t)0, cnt));
  LRF_TRY(launch(k_ms_mark, nbv, MS_NT, st, a->points, M, g, w.cell_bits, w.flag));
  LRF_TRY(launch(k_ms_count_words, blocks_for((long long)w.words_c, MS_NT), MS_NT, st, w.cell_bits, w.pre_c, w.wg_c, w.words_c));
  LRF_TRY(launch(k_points_scan, 1, PTS_SCAN_NT, st, w.wg_c, w.words_c / KEEP_GROUP, cnt + 2));
  LRF_TRY(launch(k_ms_accumulate, nbv, MS_NT, st, a->points, a->rgb8, M, g, w.cell_bits, w.pre_c, w.wg_c, w.S, w.nC, w.cell_of, cluster_of));
  return launch(k_cl_voxel_write, blocks_for(M, CL_NT), CL_NT, st, g, w.S, w.nC, w.cell_of, cnt, (long long)M, points_out, rgb8_out,
                count_out);
}
