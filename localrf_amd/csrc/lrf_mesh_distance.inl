// lrf_mesh_distance.inl -- the closest point of an indexed triangle mesh for a batch of query points, surface samples of a mesh,
// and a distance tensor summarised (included by lrf_render.hip after lrf_mesh_smooth.inl, whose sm_key and k_sm_copy it reuses;
// the scan and the wave-leader counts are lrf_compact.inl's, the host helpers lrf_host.inl's).  Unsigned distance only.  The output bytes are a
// fixed function of the input: exact minima with an index tie-break, integer sums, no float atomics.
//
// Every function below with contraction off; "fp64" means every operation rounded on its own, in the order written.
//   1. faces.  Face f = (i0, i1, i2) with an index outside [0, Nv) is never dereferenced; it is skipped and counted
//      (bad_index_faces).  A face with a corner coordinate that is not finite is skipped and counted (nonfinite_faces).  Every
//      other face is used, zero-area ones too: a face with collinear corners is the segment it is, one with equal corners the
//      point.
//   2. the pair (p, face): A, B, C, P = the fp32 corners and the point in fp64 (exact).  ab = B - A, bc = C - B, ca = A - C,
//      ac = C - A, ap = P - A, bp = P - B, cp = P - C.
//      seg(X, e, xp): ee = (e0 e0 + e1 e1) + e2 e2, pe = (xp0 e0 + xp1 e1) + xp2 e2, t = pe / ee when ee > 0, else 0; t < 0
//      becomes 0, t > 1 becomes 1; r_k = xp_k - t e_k; d2 = (r0 r0 + r1 r1) + r2 r2; closest point X_k + t e_k.
//      n = ab x ac = (ab1 ac2 - ab2 ac1, ab2 ac0 - ab0 ac2, ab0 ac1 - ab1 ac0), nn = (n0 n0 + n1 n1) + n2 n2.
//      side(e, xp) = (((e1 xp2 - e2 xp1) n0 + (e2 xp0 - e0 xp2) n1) + (e0 xp1 - e1 xp0) n2).
//      The plane term is taken when nn > 0 and side(ab, ap), side(bc, bp), side(ca, cp) are all >= 0: dn = (ap0 n0 + ap1 n1) +
//      ap2 n2, d2 = (dn dn) / nn, closest point P_k - (dn / nn) n_k.
//      The pair's d2 is seg(A, ab, ap)'s; seg(B, bc, bp)'s when strictly smaller; seg(C, ca, cp)'s when strictly smaller; the
//      plane term's when taken and strictly smaller: of equal segment terms the first in the order ab, bc, ca stays, and a
//      segment term stays against an equal plane term.  The closest point is the chosen term's, each coordinate rounded once
//      to fp32.  fp32 inputs cannot overflow any of this in fp64 (the largest intermediate is below 1e235) and no division has
//      a zero divisor, so d2 is never NaN.  The minimum is continuous across the inside / outside decision: on an edge the
//      plane term and that edge's segment term agree.
//   3. the grid.  box = the per-axis minima and maxima of the used faces' corners; cell > 0; dims_k = floor((hi_k - lo_k) /
//      cell) + 1 (the host's arithmetic).  cell_k(x) = floor(((double)x - lo_k) / cell), then clamped to [0, dims_k - 1]
//      (NaN: 0).  A used face is listed in every cell of the box cell(min corner) .. cell(max corner) per axis: cell_k is
//      monotone in x, so every point of the face lies in a cell that lists it.  The order of a cell's list is left to an atomic
//      cursor: its only consumer is the minimum of item 4, which does not depend on the order.
//   4. the query.  A point with a coordinate that is not finite: distance NaN, face -1, closest NaN.  Otherwise c = cell(p) and
//      the lane walks the Chebyshev shells r = 0, 1, 2, ... of cells around c, shell cells only, cut to the grid, evaluates
//      item 2 for every face listed in every visited cell and keeps the lexicographic minimum of (d2, f): equal distances go to
//      the smallest face index.  A face met in several cells is evaluated again, which changes nothing.  After shell r it
//      stops when, with bound = ((double)r cell) (1 - 2^-20): the best d2 < bound bound; or r >= max_k max(c_k, dims_k - 1 -
//      c_k) (the visited cube covers the grid); or bound > max_distance.
//      WHY THE BOUND HOLDS.  Let p' be p clamped onto the grid's box; c is p's cell and the clamped index is p''s.  After shell r
//      every face listed in a cell of the cube [c - r, c + r]^3 has been evaluated.  A face not listed there has, on some axis,
//      all its cells beyond the cube, so every point x of it is at least r cells from p' on that axis: |x - p'| >= r cell.
//      Clamping onto the box cannot increase a per-axis distance to a point inside the box, and every face lies inside it, so
//      |x - p| >= |x - p'| on every axis: the bound holds for points outside the grid too.  The cell expression's rounding
//      moves a cell border by an error of order 1e-10 cells at most (dims < 2^31 cells of 53-bit quotients); the factor
//      1 - 2^-20 on the bound covers it.  So an unvisited face has d2 > bound^2 > the best d2 and can neither win nor tie, and
//      when bound > max_distance every unvisited face lies beyond max_distance.
//      A result with d2 > max_distance max_distance (fp64, one product) is dropped after the search, so the output is a
//      function of (mesh, point, max_distance) alone: not of cell, the launch geometry or the stream.  No face in reach, or none
//      at all: distance +inf, face -1, closest NaN.  Otherwise distance = (float)sqrt(d2), an fp64 square root, face = f and
//      closest = item 2's closest point of (p, f), evaluated again with the same instructions.
//   5. surface samples.  Per used face the corners are rotated so that the one with the smallest (x bits, y bits, z bits), as
//      unsigned words in that order, comes first (equal corners: the earliest; such a face has no area and no sample).  With
//      mix(x): x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16 and hash3(a, b, c) = mix(mix(mix(a +
//      0x9e3779b9) ^ b) ^ c), all modulo 2^32: H = hash3 of the three corners' hash3(x bits, y bits, z bits) in rotated order.
//      n = ab x ac as in item 2 on the rotated corners, area = 0.5 sqrt(nn); count = floor(area / (spacing spacing) + H 2^-32):
//      stochastic rounding by a hash of the corners' bits, so the expected count is area / spacing^2 exactly, and neither the
//      face's index nor which corner the face starts at enters.  A count above 2^21 is refused (the host raises).
//      Sample k = 0 .. count - 1: U = mix(H ^ 0x68bc21eb) + (k + 1) 0xC13FA9A9, V = mix(H ^ 0x02e5be93) + (k + 1) 0x91E10DA5
//      modulo 2^32 (the additive recurrence of the plastic constant), u = U 2^-32, v = V 2^-32, folded into the triangle:
//      u + v > 1 -> (1 - u, 1 - v); point_k = (A_k + u ab_k) + v ac_k in fp64, rounded to fp32.  Samples come out in face order,
//      then k.
//   6. the summary of a distance tensor d [N] with thresholds tau_j (at most 8) and a unit: int64 words 0: finite entries, 1:
//      infinite ones (beyond max_distance), 2: NaN, 3: sum over the finite entries of llrint(min(d / unit, 8) 2^24) with the
//      quotient and the minimum in fp32, 4: the sum of llrint(x x 2^24), x that clamped quotient in fp64, 5: the largest bits of
//      a finite entry >= 0 (-0 as +0; 0 without one), 6, 7: 0, 8 + j: the finite entries with d <= tau_j in fp32.  CLAMP 8 and
//      SCALE 2^24: at most 2^27 and 2^30 per entry, 2^58 and 2^61 over 2^31 entries.
//
// Work distribution.  Index: k_md_bounds and k_md_fill one lane per face; a face's lane walks its whole cell box (a single face
// spanning the grid serialises one lane over every cell: the default cell keeps boxes at a few cells).  k_md_fill runs twice:
// without a list it counts (an int32 atomicAdd per overlapped cell: integer adds, the same counts on every run), k_points_scan
// turns the counts into starts and leaves the 64-bit entry total, and with the list k_md_fill's cursor starts at a copy of the
// starts and ends as the cell's end.  k_md_closest: one lane per point, no atomics, no LDS, no scratch.  k_md_sample_count / k_points_scan / k_md_sample_emit: one lane per face.
// k_md_summary: a workgroup per MD_NT MD_PX values, shuffle sums, one 64-bit integer atomic per counter and wave.
//
// No waiting: every loop is bounded by the grid, a cell box, a sample count or a list length read once; atomics are single
// instructions that are never retried; no lane, wave or workgroup waits on another.
namespace lrf {

constexpr int MD_NT = 256;
constexpr double MD_SLACK = 1.0 - 1.0 / 1048576.0;                  // 1 - 2^-20
constexpr int MD_FACE_SAMPLES = 1 << 21;                            // 1024 of them fit the scan's 32-bit block sums
constexpr int MD_PX = 8;                                            // values per lane of k_md_summary
constexpr int MD_WORDS = 16;
constexpr float MD_CLAMP = 8.0f;
constexpr double MD_SCALE = 16777216.0;                             // 2^24
constexpr int MD_NO_FACE = 0x7fffffff;

struct MdMesh { const float* vertices; const int* faces; int Nv, Nf; };
struct MdGrid { double lo[3]; double cell; int dims[3]; };

// item 1 -> 0: x holds the corners; 1: an index outside [0, Nv); 2: a coordinate not finite
__device__ __forceinline__ int md_face(const MdMesh& m, long long f, float (&x)[3][3]) {
  const int idx[3] = {m.faces[3 * f], m.faces[3 * f + 1], m.faces[3 * f + 2]};
  if (!(in_range(idx[0], m.Nv) && in_range(idx[1], m.Nv) && in_range(idx[2], m.Nv))) return 1;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      x[k][c] = m.vertices[3 * (size_t)idx[k] + c];
      finite = finite && (__float_as_uint(x[k][c]) & 0x7FFFFFFFu) < 0x7F800000u;
    }
  return finite ? 0 : 2;
}

// item 2's seg -> d2; q: the closest point
__device__ __forceinline__ double md_seg(const double (&X)[3], const double (&e)[3], const double (&xp)[3], double (&q)[3]) {
#pragma clang fp contract(off)
  const double ee = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
  const double pe = (xp[0] * e[0] + xp[1] * e[1]) + xp[2] * e[2];
  double t = ee > 0.0 ? pe / ee : 0.0;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  double r[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double te = t * e[k];
    r[k] = xp[k] - te;
    q[k] = X[k] + te;
  }
  return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
}

__device__ __forceinline__ void md_cross(const double (&a)[3], const double (&b)[3], double (&n)[3]) {
#pragma clang fp contract(off)
  n[0] = a[1] * b[2] - a[2] * b[1];
  n[1] = a[2] * b[0] - a[0] * b[2];
  n[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ double md_side(const double (&e)[3], const double (&xp)[3], const double (&n)[3]) {
#pragma clang fp contract(off)
  double c[3];
  md_cross(e, xp, c);
  return (c[0] * n[0] + c[1] * n[1]) + c[2] * n[2];
}

// item 2 -> d2 of (p, the face with corners x); q: the closest point in fp64
__device__ __forceinline__ double md_pair(const float (&p)[3], const float (&x)[3][3], double (&q)[3]) {
#pragma clang fp contract(off)
  double A[3], B[3], Cc[3], P[3], ab[3], bc[3], ca[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    A[k] = (double)x[0][k]; B[k] = (double)x[1][k]; Cc[k] = (double)x[2][k]; P[k] = (double)p[k];
    ab[k] = B[k] - A[k]; bc[k] = Cc[k] - B[k]; ca[k] = A[k] - Cc[k]; ac[k] = Cc[k] - A[k];
    ap[k] = P[k] - A[k]; bp[k] = P[k] - B[k]; cp[k] = P[k] - Cc[k];
  }
  double t[3];
  double d2 = md_seg(A, ab, ap, q);
  const double d_bc = md_seg(B, bc, bp, t);
  if (d_bc < d2) { d2 = d_bc; q[0] = t[0]; q[1] = t[1]; q[2] = t[2]; }
  const double d_ca = md_seg(Cc, ca, cp, t);
  if (d_ca < d2) { d2 = d_ca; q[0] = t[0]; q[1] = t[1]; q[2] = t[2]; }
  double n[3];
  md_cross(ab, ac, n);
  const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  if (nn > 0.0 && md_side(ab, ap, n) >= 0.0 && md_side(bc, bp, n) >= 0.0 && md_side(ca, cp, n) >= 0.0) {
    const double dn = (ap[0] * n[0] + ap[1] * n[1]) + ap[2] * n[2];
    const double d_pl = (dn * dn) / nn;
    if (d_pl < d2) {
      const double s = dn / nn;
      d2 = d_pl;
#pragma unroll
      for (int k = 0; k < 3; ++k) q[k] = P[k] - s * n[k];
    }
  }
  return d2;
}

// item 3's cell_k
__device__ __forceinline__ int md_cell(float x, double lo, double cell, int dim) {
#pragma clang fp contract(off)
  const double t = floor(((double)x - lo) / cell);
  return t > 0.0 ? (t < (double)(dim - 1) ? (int)t : dim - 1) : 0;  // NaN -> 0
}

// the cell box of a face's corners
__device__ __forceinline__ void md_box(const MdGrid& g, const float (&x)[3][3], int (&c0)[3], int (&c1)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c0[k] = md_cell(fminf(fminf(x[0][k], x[1][k]), x[2][k]), g.lo[k], g.cell, g.dims[k]);
    c1[k] = md_cell(fmaxf(fmaxf(x[0][k], x[1][k]), x[2][k]), g.lo[k], g.cell, g.dims[k]);
  }
}

// out: int64 [8] = bad_index_faces, nonfinite_faces, used_faces, 0, then six int32 (the keys of lo, of hi), 0
__global__ __launch_bounds__(64) void k_md_bounds_init(unsigned long long* __restrict__ out) {
  const int i = threadIdx.x;
  if (i < 8) out[i] = 0ull;
  __syncthreads();
  int* keys = reinterpret_cast<int*>(out + 4);
  if (i < 3) keys[i] = 0x7fffffff;
  else if (i < 6) keys[i] = -0x7fffffff - 1;
}

__global__ __launch_bounds__(MD_NT) void k_md_bounds(MdMesh m, unsigned long long* __restrict__ out) {
  const long long f = (long long)blockIdx.x * MD_NT + threadIdx.x;
  float x[3][3];
  const int kind = f < m.Nf ? md_face(m, f, x) : -1;
  wave_count(&out[0], kind == 1);
  wave_count(&out[1], kind == 2);
  wave_count(&out[2], kind == 0);
  const bool ok = kind == 0;
  const unsigned long long good = __ballot(ok);
  int* keys = reinterpret_cast<int*>(out + 4);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int lo = 0x7fffffff, hi = -0x7fffffff - 1;
    if (ok) {
      lo = sm_key(fminf(fminf(x[0][k], x[1][k]), x[2][k]));
      hi = sm_key(fmaxf(fmaxf(x[0][k], x[1][k]), x[2][k]));
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63) == 0 && good) { atomicMin(&keys[k], lo); atomicMax(&keys[3 + k], hi); }
  }
}

__global__ __launch_bounds__(MD_NT) void k_md_zero(unsigned* __restrict__ a, long long n) {
  const long long i = (long long)blockIdx.x * MD_NT + threadIdx.x;
  if (i < n) a[i] = 0u;
}

// list == null: the count pass (cursor = the counts); else the fill pass (cursor starts at the cell's start)
__global__ __launch_bounds__(MD_NT) void k_md_fill(MdMesh m, MdGrid g, unsigned* __restrict__ cursor, int* __restrict__ list,
                                                   long long entries) {
  const long long f = (long long)blockIdx.x * MD_NT + threadIdx.x;
  float x[3][3];
  if (f >= m.Nf || md_face(m, f, x) != 0) return;
  int c0[3], c1[3];
  md_box(g, x, c0, c1);
  for (int z = c0[2]; z <= c1[2]; ++z)
    for (int y = c0[1]; y <= c1[1]; ++y) {
      const long long row = ((long long)z * g.dims[1] + y) * g.dims[0];
      for (int i = c0[0]; i <= c1[0]; ++i) {
        const unsigned at = atomicAdd(&cursor[row + i], 1u);
        if (list && (long long)at < entries) list[at] = (int)f;
      }
    }
}

struct MdQuery {
  MdMesh m; MdGrid g;
  const unsigned* starts; const unsigned* ends; const int* list; long long entries;
  const float* points; long long N;
  double max_distance;
};

// the faces listed in cell ci against p
__device__ __forceinline__ void md_visit(const MdQuery& q, long long ci, const float (&p)[3], double& best, int& bf) {
  const unsigned s = q.starts[ci];
  unsigned e = q.ends[ci];
  if ((long long)e > q.entries) e = (unsigned)q.entries;
  for (unsigned j = s; j < e; ++j) {
    const int f = q.list[j];
    float x[3][3];
    double t[3];
    if (!in_range(f, q.m.Nf) || md_face(q.m, f, x) != 0) continue;  // cannot happen while the mesh is the one indexed
    const double d2 = md_pair(p, x, t);
    if (d2 < best || (d2 == best && f < bf)) { best = d2; bf = f; }
  }
}

__global__ __launch_bounds__(MD_NT) void k_md_closest(MdQuery q, float* __restrict__ distance, int* __restrict__ face,
                                                      float* __restrict__ closest) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * MD_NT + threadIdx.x;
  if (i >= q.N) return;
  const float nan = __uint_as_float(0x7FC00000u);
  float p[3];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p[k] = q.points[3 * i + k];
    finite = finite && (__float_as_uint(p[k]) & 0x7FFFFFFFu) < 0x7F800000u;
  }
  double best = __longlong_as_double(0x7FF0000000000000ll);
  int bf = MD_NO_FACE;
  if (finite) {
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
            for (int x = x0; x <= x1; ++x) md_visit(q, row + x, p, best, bf);
          } else {                                                  // r > 0 here: the two cells of the row that lie on the shell
            if (c[0] - r >= 0) md_visit(q, row + (c[0] - r), p, best, bf);
            if (c[0] + r <= d0 - 1) md_visit(q, row + (c[0] + r), p, best, bf);
          }
        }
      const double bound = ((double)r * q.g.cell) * MD_SLACK;
      if (best < bound * bound || r >= rmax || bound > q.max_distance) break;
    }
  }
  const bool hit = bf != MD_NO_FACE && !(best > q.max_distance * q.max_distance);
  distance[i] = !finite ? nan : (hit ? (float)sqrt(best) : __uint_as_float(0x7F800000u));
  face[i] = hit ? bf : -1;
  if (!closest) return;
  float cl[3] = {nan, nan, nan};
  if (hit) {
    float x[3][3];
    double t[3];
    md_face(q.m, bf, x);                                            // a winner is a used face
    md_pair(p, x, t);
    cl[0] = (float)t[0]; cl[1] = (float)t[1]; cl[2] = (float)t[2];
  }
  closest[3 * i] = cl[0]; closest[3 * i + 1] = cl[1]; closest[3 * i + 2] = cl[2];
}

// ------------------------------------------------------------------------------------------------ item 5
__device__ __forceinline__ unsigned md_mix(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __forceinline__ unsigned md_hash3(unsigned a, unsigned b, unsigned c) {
  return md_mix(md_mix(md_mix(a + 0x9e3779b9u) ^ b) ^ c);
}

struct MdSample { double A[3], ab[3], ac[3]; unsigned H; int count; bool over; };

// x: a used face's corners -> the rotated corner and edges, the hash and the sample count
__device__ __forceinline__ MdSample md_sample_face(const float (&x)[3][3], double s2) {
#pragma clang fp contract(off)
  unsigned b[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) b[k][c] = __float_as_uint(x[k][c]);
  int first = 0;
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    const bool less = b[k][0] != b[first][0] ? b[k][0] < b[first][0]
                                             : (b[k][1] != b[first][1] ? b[k][1] < b[first][1] : b[k][2] < b[first][2]);
    if (less) first = k;
  }
  const int i1 = first == 2 ? 0 : first + 1, i2 = i1 == 2 ? 0 : i1 + 1;
  MdSample s;
  s.H = md_hash3(md_hash3(b[first][0], b[first][1], b[first][2]), md_hash3(b[i1][0], b[i1][1], b[i1][2]),
                 md_hash3(b[i2][0], b[i2][1], b[i2][2]));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s.A[k] = (double)x[first][k];
    s.ab[k] = (double)x[i1][k] - s.A[k];
    s.ac[k] = (double)x[i2][k] - s.A[k];
  }
  double n[3];
  md_cross(s.ab, s.ac, n);
  const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  const double area = 0.5 * sqrt(nn);
  const double y = floor(area / s2 + (double)s.H * (1.0 / 4294967296.0));
  s.over = !(y <= (double)MD_FACE_SAMPLES);
  s.count = s.over ? 0 : (int)y;
  return s;
}

// info: int64 [4] = the total (left by the scan), bad_index_faces, nonfinite_faces, faces above MD_FACE_SAMPLES
__global__ __launch_bounds__(MD_NT) void k_md_sample_count(MdMesh m, double s2, unsigned* __restrict__ counts,
                                                           unsigned long long* __restrict__ info) {
  const long long f = (long long)blockIdx.x * MD_NT + threadIdx.x;
  float x[3][3];
  const int kind = f < m.Nf ? md_face(m, f, x) : -1;
  bool over = false;
  if (f < m.Nf) {
    unsigned n = 0;
    if (kind == 0) {
      const MdSample s = md_sample_face(x, s2);
      n = (unsigned)s.count;
      over = s.over;
    }
    counts[f] = n;
  }
  wave_count(&info[1], kind == 1);
  wave_count(&info[2], kind == 2);
  wave_count(&info[3], over);
}

__global__ __launch_bounds__(MD_NT) void k_md_sample_emit(MdMesh m, double s2, const unsigned* __restrict__ offsets, long long M,
                                                          float* __restrict__ points, int* __restrict__ face) {
#pragma clang fp contract(off)
  const long long f = (long long)blockIdx.x * MD_NT + threadIdx.x;
  float x[3][3];
  if (f >= m.Nf || md_face(m, f, x) != 0) return;
  const MdSample s = md_sample_face(x, s2);
  const long long base = offsets[f];
  const unsigned su = md_mix(s.H ^ 0x68bc21ebu), sv = md_mix(s.H ^ 0x02e5be93u);
  for (int k = 0; k < s.count; ++k) {
    const long long row = base + k;
    if (row >= M) return;
    const unsigned U = su + (unsigned)(k + 1) * 0xC13FA9A9u, V = sv + (unsigned)(k + 1) * 0x91E10DA5u;
    double u = (double)U * (1.0 / 4294967296.0), v = (double)V * (1.0 / 4294967296.0);
    if (u + v > 1.0) { u = 1.0 - u; v = 1.0 - v; }
#pragma unroll
    for (int c = 0; c < 3; ++c) points[3 * row + c] = (float)((s.A[c] + u * s.ab[c]) + v * s.ac[c]);
    face[row] = (int)f;
  }
}

// ------------------------------------------------------------------------------------------------ item 6
struct MdSummary { const float* d; long long N; int n_tau; float tau[LRF_DISTANCE_MAX_THRESHOLDS]; float unit; };

__global__ __launch_bounds__(MD_NT) void k_md_summary(MdSummary g, unsigned long long* __restrict__ words) {
#pragma clang fp contract(off)
  unsigned n_fin = 0, n_inf = 0, n_nan = 0, top = 0, within[LRF_DISTANCE_MAX_THRESHOLDS];
  unsigned long long sum1 = 0, sum2 = 0;
#pragma unroll
  for (int t = 0; t < LRF_DISTANCE_MAX_THRESHOLDS; ++t) within[t] = 0;
#pragma unroll
  for (int k = 0; k < MD_PX; ++k) {
    const long long i = ((long long)blockIdx.x * MD_PX + k) * MD_NT + threadIdx.x;
    if (i >= g.N) continue;
    const float d = g.d[i];
    const unsigned mag = __float_as_uint(d) & 0x7FFFFFFFu;
    if (mag > 0x7F800000u) { ++n_nan; continue; }
    if (mag == 0x7F800000u) { ++n_inf; continue; }
    ++n_fin;
    const double x = (double)fminf(d / g.unit, MD_CLAMP);
    sum1 += (unsigned long long)llrint(x * MD_SCALE);
    sum2 += (unsigned long long)llrint((x * x) * MD_SCALE);
    if (d >= 0.0f) top = max(top, mag);                            // -0 counts as +0
#pragma unroll
    for (int t = 0; t < LRF_DISTANCE_MAX_THRESHOLDS; ++t)
      if (t < g.n_tau && d <= g.tau[t]) ++within[t];
  }
  n_fin = wave_sum(n_fin); n_inf = wave_sum(n_inf); n_nan = wave_sum(n_nan);
  sum1 = wave_sum(sum1); sum2 = wave_sum(sum2);
  top = wave_max(top);
#pragma unroll
  for (int t = 0; t < LRF_DISTANCE_MAX_THRESHOLDS; ++t) within[t] = wave_sum(within[t]);
  if ((threadIdx.x & 63) == 0) {
    if (n_fin) atomicAdd(&words[0], (unsigned long long)n_fin);
    if (n_inf) atomicAdd(&words[1], (unsigned long long)n_inf);
    if (n_nan) atomicAdd(&words[2], (unsigned long long)n_nan);
    if (sum1) atomicAdd(&words[3], sum1);
    if (sum2) atomicAdd(&words[4], sum2);
    if (top) atomicMax(&words[5], (unsigned long long)top);
#pragma unroll
    for (int t = 0; t < LRF_DISTANCE_MAX_THRESHOLDS; ++t)
      if (within[t]) atomicAdd(&words[8 + t], (unsigned long long)within[t]);
  }
}

// ------------------------------------------------------------------------------------------------ host side
// the grid's arrays: a start and an end per cell
struct MdGridWs { unsigned* starts; unsigned* ends; size_t bytes; };
static MdGridWs md_carve(void* grid, long long cells) {
  Carver c(grid);
  MdGridWs w;
  w.starts = c.take<unsigned>((size_t)cells);
  w.ends = c.take<unsigned>((size_t)cells);
  w.bytes = c.bytes();
  return w;
}

// the cells of dims, 0 when a dimension is < 1 or the product reaches 2^31
static long long md_cells(const int32_t (&dims)[3]) {
  long long n = 1;
  for (int k = 0; k < 3; ++k) {
    if (dims[k] < 1) return 0;
    n *= dims[k];
    if (n >= (1ll << 31)) return 0;
  }
  return n;
}

// the members every entry point over an index reads; fills m, g and cells
static int md_index_args(const char* who, const LrfMeshIndex* a, MdMesh& m, MdGrid& g, long long& cells) {
  if (!a) return refuse(who, "null argument");
  if (!mesh_shape(a->Nv, a->Nf) || a->Nf < 1) return refuse(who, "need 1 <= Nv < 2^31 and 1 <= Nf < 2^31");
  cells = md_cells(a->dims);
  if (!cells) return refuse(who, "need dims >= 1 with fewer than 2^31 cells");
  if (!(a->cell > 0.0) || !is_finite(a->cell) || !is_finite(a->lo[0]) || !is_finite(a->lo[1]) || !is_finite(a->lo[2]))
    return refuse(who, "need a finite cell > 0 and a finite lo");
  if (!a->vertices || !a->faces || !a->grid) return refuse(who, "null argument");
  if (misaligned(3, a->vertices, a->faces, a->list)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, a->grid)) return refuse(who, "grid must be 8-byte aligned");
  m = {a->vertices, a->faces, (int)a->Nv, (int)a->Nf};
  g.cell = a->cell;
  for (int k = 0; k < 3; ++k) { g.lo[k] = a->lo[k]; g.dims[k] = a->dims[k]; }
  return 0;
}

static int md_mesh_args(const char* who, const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, MdMesh& m) {
  if (!mesh_shape(Nv, Nf)) return refuse(who, "need 1 <= Nv < 2^31 and 0 <= Nf < 2^31");
  if (Nf > 0 && (!vertices || !faces)) return refuse(who, "null argument");
  if (misaligned(3, vertices, faces)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  m = {vertices, faces, (int)Nv, (int)Nf};
  return 0;
}

}  // namespace lrf

extern "C" int lrf_mesh_index_bounds(const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, int64_t* out, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_index_bounds";
  MdMesh m;
  LRF_TRY(md_mesh_args(who, vertices, faces, Nv, Nf, m));
  if (!out) return refuse(who, "null argument");
  if (misaligned(7, out)) return refuse(who, "out must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
  LRF_TRY(launch(k_md_bounds_init, 1, 64, st, o));
  if (Nf) LRF_TRY(launch(k_md_bounds, blocks_for(Nf, MD_NT), MD_NT, st, m, o));
  return 0;
}

extern "C" size_t lrf_mesh_index_workspace_bytes(int64_t cells) {
  return cells >= 1 && cells < (1ll << 31) ? lrf::md_carve(nullptr, cells).bytes : 0;
}

extern "C" int lrf_mesh_index_build(const LrfMeshIndex* a, int64_t* total, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_index_build";
  MdMesh m;
  MdGrid g;
  long long cells = 0;
  LRF_TRY(md_index_args(who, a, m, g, cells));
  if (!a->list && !total) return refuse(who, "the count pass (list null) needs total");
  if (a->list && (a->entries < 0 || a->entries >= (1ll << 31))) return refuse(who, "need 0 <= entries < 2^31");
  if (misaligned(7, total)) return refuse(who, "total must be 8-byte aligned");
  const MdGridWs w = md_carve(a->grid, cells);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!a->list) {
    LRF_TRY(launch(k_md_zero, blocks_for(cells, MD_NT), MD_NT, st, w.starts, cells));
    LRF_TRY(launch(k_md_fill, blocks_for(m.Nf, MD_NT), MD_NT, st, m, g, w.starts, (int*)nullptr, 0ll));
    return launch(k_points_scan, 1, PTS_SCAN_NT, st, w.starts, (int)cells, reinterpret_cast<long long*>(total));
  }
  LRF_TRY(launch(k_sm_copy, blocks_for(cells, SM_NT), SM_NT, st, w.starts, w.ends, cells));
  return launch(k_md_fill, blocks_for(m.Nf, MD_NT), MD_NT, st, m, g, w.ends, a->list, a->entries);
}

extern "C" int lrf_mesh_closest(const LrfMeshIndex* a, const float* points, int64_t N, double max_distance, float* distance,
                                int32_t* face, float* closest, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_closest";
  MdQuery q;
  memset(&q, 0, sizeof(q));
  long long cells = 0;
  LRF_TRY(md_index_args(who, a, q.m, q.g, cells));
  if (!a->list || a->entries < 0 || a->entries >= (1ll << 31)) return refuse(who, "need the list and 0 <= entries < 2^31");
  if (N < 1 || N >= (1ll << 31)) return refuse(who, "need 1 <= N < 2^31");
  if (!(max_distance >= 0.0)) return refuse(who, "max_distance must be >= 0 (infinity allowed)");
  if (!points || !distance || !face) return refuse(who, "null argument");
  if (misaligned(3, points, distance, face, closest)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  const MdGridWs w = md_carve(a->grid, cells);
  q.starts = w.starts; q.ends = w.ends; q.list = a->list; q.entries = a->entries;
  q.points = points; q.N = N; q.max_distance = max_distance;
  return launch(k_md_closest, blocks_for(N, MD_NT), MD_NT, reinterpret_cast<hipStream_t>(stream), q, distance, face, closest);
}

extern "C" int lrf_mesh_sample_count(const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, double spacing,
                                     uint32_t* offsets, int64_t* info, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_sample_count";
  MdMesh m;
  LRF_TRY(md_mesh_args(who, vertices, faces, Nv, Nf, m));
  if (Nf < 1) return refuse(who, "need Nf >= 1");
  if (!(spacing > 0.0) || !is_finite(spacing)) return refuse(who, "spacing must be finite and > 0");
  if (!offsets || !info) return refuse(who, "null argument");
  if (misaligned(3, offsets)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, info)) return refuse(who, "info must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
  LRF_TRY(launch(k_ag_zero, 1, RS_NT, st, inf, 4ll));
  LRF_TRY(launch(k_md_sample_count, blocks_for(Nf, MD_NT), MD_NT, st, m, spacing * spacing, offsets, inf));
  return launch(k_points_scan, 1, PTS_SCAN_NT, st, offsets, (int)Nf, reinterpret_cast<long long*>(info));
}

extern "C" int lrf_mesh_sample_emit(const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, double spacing,
                                    const uint32_t* offsets, int64_t M, float* points, int32_t* face, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_sample_emit";
  MdMesh m;
  LRF_TRY(md_mesh_args(who, vertices, faces, Nv, Nf, m));
  if (Nf < 1 || M < 1 || M >= (1ll << 31)) return refuse(who, "need Nf >= 1 and 1 <= M < 2^31");
  if (!(spacing > 0.0) || !is_finite(spacing)) return refuse(who, "spacing must be finite and > 0");
  if (!offsets || !points || !face) return refuse(who, "null argument");
  if (misaligned(3, offsets, points, face)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  return launch(k_md_sample_emit, blocks_for(Nf, MD_NT), MD_NT, reinterpret_cast<hipStream_t>(stream), m, spacing * spacing, offsets, M,
                points, face);
}

extern "C" int lrf_distance_summary(const float* distance, int64_t N, const float* thresholds, int32_t n_thresholds, float unit,
                                    int64_t* words, void* stream) {
  using namespace lrf;
  const char* who = "lrf_distance_summary";
  if (N < 0 || N >= (1ll << 31)) return refuse(who, "need 0 <= N < 2^31");
  if (n_thresholds < 0 || n_thresholds > LRF_DISTANCE_MAX_THRESHOLDS)
    return refuse(who, "n_thresholds must lie in [0, LRF_DISTANCE_MAX_THRESHOLDS]");
  if ((N && !distance) || !words || (n_thresholds && !thresholds)) return refuse(who, "null argument");
  if (!(unit > 0.0f) || !is_finite((double)unit)) return refuse(who, "unit must be finite and > 0");
  for (int k = 0; k < n_thresholds; ++k)
    if (!(thresholds[k] > 0.0f) || !is_finite((double)thresholds[k])) return refuse(who, "a threshold must be finite and > 0");
  if (misaligned(3, distance)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, words)) return refuse(who, "words must be 8-byte aligned");
  MdSummary g;
  memset(&g, 0, sizeof(g));
  g.d = distance; g.N = N; g.n_tau = n_thresholds; g.unit = unit;
  for (int k = 0; k < n_thresholds; ++k) g.tau[k] = thresholds[k];
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* w = reinterpret_cast<unsigned long long*>(words);
  LRF_TRY(launch(k_ag_zero, 1, RS_NT, st, w, (long long)MD_WORDS));
  if (N) LRF_TRY(launch(k_md_summary, blocks_for(N, MD_NT * MD_PX), MD_NT, st, g, w));
  return 0;
}
