// lrf_align.inl -- what a registration needs around lrf_mesh_closest: a similarity applied to points, the exact moments of
// corresponding pairs, and the normal equations of one linearised point-to-plane step, against a mesh's faces or against the
// normals stored for a cloud's points (included by lrf_render.hip after lrf_mesh_distance.inl, whose MdMesh, md_face and
// md_cross it reuses; k_ag_zero is lrf_mesh_raster.inl's, the reductions lrf_common.h's, the host helpers lrf_host.inl's).
// The fit itself, a 3 x 3 SVD or a 7 x 7 solve, is the host's (localrf_amd/alignment.py).  The output bytes are a fixed
// function of the input: integer sums, no float atomics.
//
// Every function below with contraction off; "fp64" means every operation rounded on its own, in the order written.
//   1. the transform.  T: 12 doubles, row-major 3 x 4.  With x, y, z the point's fp32 coordinates in fp64 (exact):
//      out_k = (float)(((T[4k] x + T[4k+1] y) + T[4k+2] z) + T[4k+3]).  A lane reads its point before it writes it: out may be
//      points.
//   2. the moments of pairs (a_i, b_i), i < N <= 2^20, in the frame (c, h), h > 0 a power of two (so the division is exact but
//      for under- and overflow).  Per coordinate t = ((double)x - c_k) / h, r = rint(t) (ties to even); the integer coordinate is
//      (long long)r.  A pair is skipped and counted, the first that applies: keep is given and keep[i] == 0 (masked); one of its
//      six coordinates is not finite (nonfinite); one of its six r has |r| >= 2^20, an infinite r among them (out_of_range).
//      words, int64 [24]: 0 the pairs summed (n), 1 out_of_range, 2 masked, 3 nonfinite, 4..6 sum a, 7..9 sum b, 10 + 3 i + j
//      sum a_i b_j, 19 sum (a0 a0 + a1 a1 + a2 a2), 20 the same of b, 21..23 zero.
//      NO OVERFLOW.  |coordinate| <= 2^20 - 1: a product is below 2^40 and 2^20 of them sum below 2^60; a squared length is
//      below 3 2^40 and 2^20 of them sum below 3 2^60 < 2^62.  N > 2^20 is refused: the caller adds the words of its chunks.
//   3. the point-to-plane step over points p_i with lrf_mesh_closest's outputs for them (closest q_i, face f_i, distance d_i),
//      i < N <= 2^20, in the frame (c, u), u > 0 a power of two, with a gate (fp32; +inf allowed).  Per point, the first that
//      applies: f_i outside [0, Nf), d_i not finite, or the face not a used one of lrf_mesh_distance.inl's item 1 (unmatched);
//      d_i > gate in fp32 (gated); with A, B, C the face's corners in fp64, ab = B - A, ac = C - A, n = ab x ac and nn =
//      (n0 n0 + n1 n1) + n2 n2 as in item 2 there: nn == 0 (degenerate); pt_k = ((double)p_k - c_k) / u, qt_k = ((double)q_k -
//      c_k) / u and not all six |.| <= 1 (out_of_range; a NaN among them too).  Otherwise m_k = n_k / sqrt(nn),
//      d_k = pt_k - qt_k, r = (m0 d0 + m1 d1) + m2 d2, and J = (pt x m, m, pt . m): J0 = pt1 m2 - pt2 m1, J1 = pt2 m0 - pt0 m2,
//      J2 = pt0 m1 - pt1 m0, J3..5 = m, J6 = (pt0 m0 + pt1 m1) + pt2 m2.  Every product below is formed once in fp64, then
//      multiplied by 2^36, then rounded by llrint (ties to even).
//      words, int64 [48]: 0 the points summed (n), 1 unmatched, 2 gated, 3 degenerate, 4 out_of_range, 5 zero, 6 sum
//      llrint((r r) 2^36), 7 + k sum llrint((J_k r) 2^36), 14.. sum llrint((J_k J_l) 2^36) for k <= l row by row ((0,0), (0,1),
//      .. (0,6), (1,1), ..: 28 words), 42..47 zero.
//      NO OVERFLOW.  |pt|, |qt| <= sqrt(3), |m| <= 1 + 2^-50: |r| <= 2 sqrt(3) (1 + 2^-50), |J_k| <= sqrt(3) (1 + 2^-50) < 3 +
//      sqrt(3).  So |r r| <= 12.1, |J_k r| <= (3 + sqrt(3)) 2 sqrt(3) < 16.4, |J_k J_l| < (3 + sqrt(3))^2 < 22.4 < 2^4.5: a term
//      is below 2^40.5, and 2^20 of them sum below 2^60.5, a factor of five under 2^63.  The exponent 36 stays.
//      A face index is tested before it is used and a corner index inside md_face: nothing outside the arrays is dereferenced,
//      whatever face holds.
//   4. item 3 against a cloud: points p_i with lrf_cloud_closest's outputs for them (closest q_i, index j_i, distance d_i) and
//      normals [M,3] fp32, one per cloud point (lrf_cloud_normals' or any other; a zero row marks a point without one).  Per
//      point, the first that applies: j_i outside [0, M) or d_i not finite (unmatched); d_i > gate in fp32 (gated); the three
//      words of normals[j_i] not all finite, or with n their fp64 values nn = (n0 n0 + n1 n1) + n2 n2 == 0 (degenerate);
//      out_of_range exactly as item 3.  Otherwise m_k = n_k / sqrt(nn) and r, J and the sums exactly as item 3: the same 48
//      words in the same layout.  k_al_plane_cloud repeats k_al_plane's lines from pt, qt on: shared through a function over s
//      they cost k_al_plane 32 more registers and 5 % of its time, so k_al_plane stays as it was, line for line.
//      NO OVERFLOW.  Item 3's argument rests on |pt|, |qt| <= sqrt(3) and |m| <= 1 + 2^-50 alone, and m is again a vector
//      divided by the root of its own squared length: it carries over word for word.  An index is tested before it is used.
//
// Work distribution.  k_al_transform: one lane per point.  k_al_pairs, k_al_plane and k_al_plane_cloud: a workgroup per AL_NT AL_PX
// points, lane t on points t, t + AL_NT, ..: consecutive lanes on consecutive points, the sums as long long in registers;
// block_sum0 over the workgroup, then thread 0 issues one 64-bit integer atomicAdd per non-zero word: at 2^20 points 512
// workgroups, about 21 000 adds on 42 addresses (per wave it would be four times that).  Integer adds commute: the words depend
// on neither scheduling, launch geometry nor the order of the points.  LDS: the helper's [words][waves] only.
//
// No waiting: every loop has AL_PX steps; atomics are single instructions that are never retried; no lane, wave or workgroup
// waits on another beyond block_sum0's one barrier.
namespace lrf {

constexpr int AL_NT = 256;
constexpr int AL_PX = 8;                                             // points per lane of the two accumulations
constexpr long long AL_MAX_N = 1ll << 20;                            // per call: items 2 and 3's overflow bounds
constexpr int AL_PAIR_WORDS = 24, AL_PAIR_SUMS = 21;
constexpr int AL_PLANE_WORDS = 48, AL_PLANE_SUMS = 42;
constexpr double AL_RANGE = 1048576.0;                               // 2^20
constexpr double AL_SCALE = 68719476736.0;                           // 2^36

struct AlT { double t[12]; };

__global__ __launch_bounds__(AL_NT) void k_al_transform(AlT T, const float* points, long long N, float* out) {
#pragma clang fp contract(off)
  const long long i = (long long)blockIdx.x * AL_NT + threadIdx.x;
  if (i >= N) return;
  const double x = (double)points[3 * i], y = (double)points[3 * i + 1], z = (double)points[3 * i + 2];
  float o[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = (float)(((T.t[4 * k] * x + T.t[4 * k + 1] * y) + T.t[4 * k + 2] * z) + T.t[4 * k + 3]);
  out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
}

// thread 0 after block_sum0: one atomic per non-zero word
template <int NV>
__device__ __forceinline__ void al_flush(const long long (&s)[NV], unsigned long long* __restrict__ words) {
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int w = 0; w < NV; ++w)
    if (s[w]) atomicAdd(&words[w], (unsigned long long)s[w]);
}

struct AlFrame { double c[3]; double h; };

__global__ __launch_bounds__(AL_NT) void k_al_pairs(AlFrame fr, const float* __restrict__ a, const float* __restrict__ b,
                                                    const unsigned char* __restrict__ keep, long long N,
                                                    unsigned long long* __restrict__ words) {
#pragma clang fp contract(off)
  __shared__ long long red[AL_PAIR_SUMS * (AL_NT / 64)];
  long long s[AL_PAIR_SUMS];
#pragma unroll
  for (int w = 0; w < AL_PAIR_SUMS; ++w) s[w] = 0;
  for (int k = 0; k < AL_PX; ++k) {
    const long long i = ((long long)blockIdx.x * AL_PX + k) * AL_NT + threadIdx.x;
    if (i >= N) break;
    if (keep && keep[i] == 0) { ++s[2]; continue; }
    float x[6];
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) { x[j] = a[3 * i + j]; x[3 + j] = b[3 * i + j]; }
#pragma unroll
    for (int j = 0; j < 6; ++j) finite = finite && (__float_as_uint(x[j]) & 0x7FFFFFFFu) < 0x7F800000u;
    if (!finite) { ++s[3]; continue; }
    long long q[6];
    bool inside = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double r = rint(((double)x[j] - fr.c[j % 3]) / fr.h);
      inside = inside && fabs(r) < AL_RANGE;
      q[j] = inside ? (long long)r : 0;
    }
    if (!inside) { ++s[1]; continue; }
    ++s[0];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      s[4 + j] += q[j];
      s[7 + j] += q[3 + j];
#pragma unroll
      for (int l = 0; l < 3; ++l) s[10 + 3 * j + l] += q[j] * q[3 + l];
    }
    s[19] += (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    s[20] += (q[3] * q[3] + q[4] * q[4]) + q[5] * q[5];
  }
  block_sum0<AL_NT>(s, red);
  al_flush(s, words);
}

struct AlPlane {
  MdMesh m;
  const float* points; const float* closest; const int* face; const float* distance;
  long long N;
  double c[3]; double u;
  float gate;
};

__global__ __launch_bounds__(AL_NT) void k_al_plane(AlPlane g, unsigned long long* __restrict__ words) {
#pragma clang fp contract(off)
  __shared__ long long red[AL_PLANE_SUMS * (AL_NT / 64)];
  long long s[AL_PLANE_SUMS];
#pragma unroll
  for (int w = 0; w < AL_PLANE_SUMS; ++w) s[w] = 0;
#pragma unroll 1
  for (int k = 0; k < AL_PX; ++k) {
    const long long i = ((long long)blockIdx.x * AL_PX + k) * AL_NT + threadIdx.x;
    if (i >= g.N) break;
    const int f = g.face[i];
    const float d = g.distance[i];
    float x[3][3];
    if (!in_range(f, g.m.Nf) || !((__float_as_uint(d) & 0x7FFFFFFFu) < 0x7F800000u) || md_face(g.m, f, x) != 0) { ++s[1]; continue; }
    if (d > g.gate) { ++s[2]; continue; }
    double ab[3], ac[3], n[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      ab[j] = (double)x[1][j] - (double)x[0][j];
      ac[j] = (double)x[2][j] - (double)x[0][j];
    }
    md_cross(ab, ac, n);
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (nn == 0.0) { ++s[3]; continue; }
    double pt[3], qt[3];
    bool inside = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      pt[j] = ((double)g.points[3 * i + j] - g.c[j]) / g.u;
      qt[j] = ((double)g.closest[3 * i + j] - g.c[j]) / g.u;
      inside = inside && fabs(pt[j]) <= 1.0 && fabs(qt[j]) <= 1.0;    // a NaN fails
    }
    if (!inside) { ++s[4]; continue; }
    const double len = sqrt(nn);
    double J[7], dd[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      J[3 + j] = n[j] / len;
      dd[j] = pt[j] - qt[j];
    }
    const double r = (J[3] * dd[0] + J[4] * dd[1]) + J[5] * dd[2];
    J[0] = pt[1] * J[5] - pt[2] * J[4];
    J[1] = pt[2] * J[3] - pt[0] * J[5];
    J[2] = pt[0] * J[4] - pt[1] * J[3];
    J[6] = (pt[0] * J[3] + pt[1] * J[4]) + pt[2] * J[5];
    ++s[0];
    s[6] += llrint((r * r) * AL_SCALE);
#pragma unroll
    for (int a = 0; a < 7; ++a) {
      s[7 + a] += llrint((J[a] * r) * AL_SCALE);
#pragma unroll
      for (int l = a; l < 7; ++l) s[14 + 7 * a - a * (a - 1) / 2 + (l - a)] += llrint((J[a] * J[l]) * AL_SCALE);
    }
  }
  block_sum0<AL_NT>(s, red);
  al_flush(s, words);
}

struct AlPlaneCloud {
  const float* points; const float* closest; const int* index; const float* distance; const float* normals;
  long long N; int M;
  double c[3]; double u;
  float gate;
};

__global__ __launch_bounds__(AL_NT) void k_al_plane_cloud(AlPlaneCloud g, unsigned long long* __restrict__ words) {
#pragma clang fp contract(off)
  __shared__ long long red[AL_PLANE_SUMS * (AL_NT / 64)];
  long long s[AL_PLANE_SUMS];
#pragma unroll
  for (int w = 0; w < AL_PLANE_SUMS; ++w) s[w] = 0;
#pragma unroll 1
  for (int k = 0; k < AL_PX; ++k) {
    const long long i = ((long long)blockIdx.x * AL_PX + k) * AL_NT + threadIdx.x;
    if (i >= g.N) break;
    const int f = g.index[i];
    const float d = g.distance[i];
    if (!in_range(f, g.M) || !((__float_as_uint(d) & 0x7FFFFFFFu) < 0x7F800000u)) { ++s[1]; continue; }
    if (d > g.gate) { ++s[2]; continue; }
    double n[3];
    bool finite = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float w = g.normals[3ll * f + j];
      finite = finite && (__float_as_uint(w) & 0x7FFFFFFFu) < 0x7F800000u;
      n[j] = (double)w;
    }
    const double nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (!finite || nn == 0.0) { ++s[3]; continue; }
    double pt[3], qt[3];
    bool inside = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      pt[j] = ((double)g.points[3 * i + j] - g.c[j]) / g.u;
      qt[j] = ((double)g.closest[3 * i + j] - g.c[j]) / g.u;
      inside = inside && fabs(pt[j]) <= 1.0 && fabs(qt[j]) <= 1.0;    // a NaN fails
    }
    if (!inside) { ++s[4]; continue; }
    const double len = sqrt(nn);
    double J[7], dd[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      J[3 + j] = n[j] / len;
      dd[j] = pt[j] - qt[j];
    }
    const double r = (J[3] * dd[0] + J[4] * dd[1]) + J[5] * dd[2];
    J[0] = pt[1] * J[5] - pt[2] * J[4];
    J[1] = pt[2] * J[3] - pt[0] * J[5];
    J[2] = pt[0] * J[4] - pt[1] * J[3];
    J[6] = (pt[0] * J[3] + pt[1] * J[4]) + pt[2] * J[5];
    ++s[0];
    s[6] += llrint((r * r) * AL_SCALE);
#pragma unroll
    for (int a = 0; a < 7; ++a) {
      s[7 + a] += llrint((J[a] * r) * AL_SCALE);
#pragma unroll
      for (int l = a; l < 7; ++l) s[14 + 7 * a - a * (a - 1) / 2 + (l - a)] += llrint((J[a] * J[l]) * AL_SCALE);
    }
  }
  block_sum0<AL_NT>(s, red);
  al_flush(s, words);
}

// x > 0, finite and a power of two
static bool al_power_of_two(double x) {
  int e;
  return x > 0.0 && is_finite(x) && frexp(x, &e) == 0.5;
}

}  // namespace lrf

extern "C" int lrf_align_transform(const double* T, const float* points, int64_t N, float* out, void* stream) {
  using namespace lrf;
  const char* who = "lrf_align_transform";
  if (N < 0 || N >= (1ll << 31)) return refuse(who, "need 0 <= N < 2^31");
  if (!T || (N && (!points || !out))) return refuse(who, "null argument");
  if (misaligned(7, T)) return refuse(who, "T must be 8-byte aligned");
  if (misaligned(3, points, out)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  AlT t;
  for (int k = 0; k < 12; ++k) {
    if (!is_finite(T[k])) return refuse(who, "T must be finite");
    t.t[k] = T[k];
  }
  if (!N) return 0;
  return launch(k_al_transform, blocks_for(N, AL_NT), AL_NT, reinterpret_cast<hipStream_t>(stream), t, points, (long long)N, out);
}

extern "C" int lrf_align_pairs(const LrfAlignFrame* fr, const float* a, const float* b, const uint8_t* keep, int64_t N, int64_t* words,
                               void* stream) {
  using namespace lrf;
  const char* who = "lrf_align_pairs";
  if (!fr || !words) return refuse(who, "null argument");
  if (N < 0 || N > AL_MAX_N) return refuse(who, "need 0 <= N <= 2^20");
  if (N && (!a || !b)) return refuse(who, "null argument");
  if (!al_power_of_two(fr->h)) return refuse(who, "h must be a positive power of two");
  if (!is_finite(fr->c[0]) || !is_finite(fr->c[1]) || !is_finite(fr->c[2])) return refuse(who, "c must be finite");
  if (misaligned(3, a, b)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, words)) return refuse(who, "words must be 8-byte aligned");
  AlFrame g;
  for (int k = 0; k < 3; ++k) g.c[k] = fr->c[k];
  g.h = fr->h;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* w = reinterpret_cast<unsigned long long*>(words);
  LRF_TRY(launch(k_ag_zero, 1, RS_NT, st, w, (long long)AL_PAIR_WORDS));
  if (N) LRF_TRY(launch(k_al_pairs, blocks_for(N, AL_NT * AL_PX), AL_NT, st, g, a, b, keep, (long long)N, w));
  return 0;
}

extern "C" int lrf_align_plane(const LrfAlignPlane* p, int64_t* words, void* stream) {
  using namespace lrf;
  const char* who = "lrf_align_plane";
  if (!p || !words) return refuse(who, "null argument");
  AlPlane g;
  memset(&g, 0, sizeof(g));
  LRF_TRY(md_mesh_args(who, p->vertices, p->faces, p->Nv, p->Nf, g.m));
  if (p->Nf < 1) return refuse(who, "need Nf >= 1");
  if (p->N < 0 || p->N > AL_MAX_N) return refuse(who, "need 0 <= N <= 2^20");
  if (p->N && (!p->points || !p->closest || !p->face || !p->distance)) return refuse(who, "null argument");
  if (!al_power_of_two(p->u)) return refuse(who, "u must be a positive power of two");
  if (!is_finite(p->c[0]) || !is_finite(p->c[1]) || !is_finite(p->c[2])) return refuse(who, "c must be finite");
  if (!(p->gate >= 0.0f)) return refuse(who, "gate must be >= 0 (infinity allowed)");
  if (misaligned(3, p->points, p->closest, p->face, p->distance)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, words)) return refuse(who, "words must be 8-byte aligned");
  g.points = p->points; g.closest = p->closest; g.face = p->face; g.distance = p->distance;
  g.N = p->N; g.u = p->u; g.gate = p->gate;
  for (int k = 0; k < 3; ++k) g.c[k] = p->c[k];
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* w = reinterpret_cast<unsigned long long*>(words);
  LRF_TRY(launch(k_ag_zero, 1, RS_NT, st, w, (long long)AL_PLANE_WORDS));
  if (p->N) LRF_TRY(launch(k_al_plane, blocks_for(p->N, AL_NT * AL_PX), AL_NT, st, g, w));
  return 0;
}

extern "C" int lrf_align_plane_cloud(const LrfAlignPlaneCloud* p, int64_t* words, void* stream) {
  using namespace lrf;
  const char* who = "lrf_align_plane_cloud";
  if (!p || !words) return refuse(who, "null argument");
  if (p->M < 1 || p->M >= (1ll << 31)) return refuse(who, "need 1 <= M < 2^31");
  if (p->N < 0 || p->N > AL_MAX_N) return refuse(who, "need 0 <= N <= 2^20");
  if (!p->normals || (p->N && (!p->points || !p->closest || !p->index || !p->distance))) return refuse(who, "null argument");
  if (!al_power_of_two(p->u)) return refuse(who, "u must be a positive power of two");
  if (!is_finite(p->c[0]) || !is_finite(p->c[1]) || !is_finite(p->c[2])) return refuse(who, "c must be finite");
  if (!(p->gate >= 0.0f)) return refuse(who, "gate must be >= 0 (infinity allowed)");
  if (misaligned(3, p->points, p->closest, p->index, p->distance, p->normals))
    return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, words)) return refuse(who, "words must be 8-byte aligned");
  AlPlaneCloud g;
  memset(&g, 0, sizeof(g));
  g.points = p->points; g.closest = p->closest; g.index = p->index; g.distance = p->distance; g.normals = p->normals;
  g.N = p->N; g.M = (int)p->M; g.u = p->u; g.gate = p->gate;
  for (int k = 0; k < 3; ++k) g.c[k] = p->c[k];
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* w = reinterpret_cast<unsigned long long*>(words);
  LRF_TRY(launch(k_ag_zero, 1, RS_NT, st, w, (long long)AL_PLANE_WORDS));
  if (p->N) LRF_TRY(launch(k_al_plane_cloud, blocks_for(p->N, AL_NT * AL_PX), AL_NT, st, g, w));
  return 0;
}
