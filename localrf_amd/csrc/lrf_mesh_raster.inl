// lrf_mesh_raster.inl -- an indexed triangle mesh rasterised into V pinhole cameras, and two depth maps compared (included by
// lrf_render.hip; it reuses to_camera and pts_finite_pos of lrf_points.inl, pinhole_x / pinhole_y of lrf_scene.inl and sm_face of
// lrf_mesh_smooth.inl; the wave-leader counts are lrf_compact.inl's, the host helpers lrf_host.inl's).  The inverse of k_tsdf_integrate: mesh -> depth at a pose, in the depth
// convention of lrf_points.inl (a multiple of the un-normalised pixel direction whose z is -1).  The output bytes are a fixed
// function of the input: one consistent ray per pixel, an exact-sign coverage test, and an integer minimum per pixel.
//
// Per frame v and face f = (i0, i1, i2), every function below with contraction off:
//   1. q_k = to_camera(M_v, vertex i_k) in fp32 (d = p - t, q = R^T d column by column: reproject's arithmetic), nz_k = -q_k.z.
//      A face with an index outside [0, Nv) is never dereferenced; it, a face with two equal indices and a face with a coordinate
//      that is not finite are skipped and counted (info[0], info[1], info[2], once per call, not per frame).  A face with all three
//      nz <= 0 lies behind the camera plane and is skipped.
//   2. per pixel (i, j) with direction (x, y, -1) = (pinhole_x(i), pinhole_y(j), -1): every corner is sheared onto the plane
//      through the camera, a_k = (q.x + q.z x, q.y + q.z y) in fp32, two operations each -- the same value for every face that
//      shares the vertex.  The edge function of the directed edge b -> c is U = ax_b ay_c - ay_b ax_c in fp64: both products of
//      fp32 values are exact, so the difference has the exact sign, is zero only on equality, and U(c -> b) = -U(b -> c) exactly.
//      A zero U takes the sign of ay_b - ay_c, then of ax_c - ax_b: the ray shifted symbolically by (eps, eps^2), the same shift for
//      every face.  Still zero: the edge is degenerate for this ray and the face is not hit.  U_0, U_1, U_2 belong to the edges
//      1 -> 2, 2 -> 0, 0 -> 1.  The pixel is covered when the three signs are equal and not zero.
//      THE COMMON SIGN s: s > 0 SEES THE SIDE THE WINDING'S NORMAL (q_1 - q_0) x (q_2 - q_0) POINTS TO -- free space for a TSDF
//      mesh -- because det[q_0, q_1, q_2] = sum q_k.z U_k = -t D and the camera is on the normal's side when the determinant is < 0.
//      cull = 1 ("back") drops the hits with s < 0, cull = 2 ("front") those with s > 0, 0 keeps both.
//   3. t = ((U_0 nz_0 + U_1 nz_1) + U_2 nz_2) / ((U_0 + U_1) + U_2) in fp64, every operation rounded on its own, then rounded
//      once to fp32.  The hit is kept when t is finite, t > 0 and d_min <= t <= d_max.  Faces that straddle the camera plane need
//      no clipping: the part behind the camera gives t <= 0.  crossings counts the kept hits of both orientations (cull does not
//      enter): even outside a closed mesh, odd inside.
//   4. visibility: key = t's bits << 32 | f; atomicMin on an unsigned 64-bit word per pixel that starts at all ones.  Positive
//      floats order as their bits and equal depths go to the smallest face index, so the minimum does not depend on the order of
//      the updates: the same bytes for every schedule, launch geometry and stream.
//   5. resolve: depth = the key's upper half (0.0 where no face was kept), face = its lower half (-1), and for the winner steps
//      1 and 2 again with the same instructions: weights_k = (float)(U_k / D) with D = (U_0 + U_1) + U_2 in fp64; rgb8 per channel
//      = ((w_0 c_0 + w_1 c_1) + w_2 c_2) in fp64 with w_k = U_k / D unrounded, then rint (ROUND TO NEAREST, TIES TO EVEN) and a
//      clamp to [0, 255].  Pixels without a hit get weights 0 and colour 0.
//
// Work distribution.  k_rs_faces: one lane per (frame, face).  Its conservative pixel box: with all nz > 0 the corners' pixel
// coordinates (reproject's u, w) widened to floor(min) - 1 .. ceil(max) + 1 and cut to the image (the shear's rounding moves an
// edge by 2^-23 of its distance from the principal point, far below the pixel of slack); the whole image when the face straddles
// the camera plane or a coordinate is NaN.  An empty box: nothing.  A box of at most small_max pixels: the lane walks it.  A larger
// one: the pair is appended to a list through an atomic cursor, advanced once per wave by the ballot's count -- the list's order
// is free, because its only consumer is the order-independent minimum (and integer adds).  k_rs_large: a fixed grid of wavefronts
// strides the list up to the device-side cursor (no read-back); an entry's box is cut into groups of 64 consecutive pixels, lanes
// across a group, and the wavefronts of grid row y take every RS_LARGE_SLICES-th group from y on, so that a face that fills the
// image is shared by 8 wavefronts.
//
// depth agreement (k_depth_agreement): two depth maps [V,H,W]; a value is valid when finite, positive and inside [d_min, d_max].
// Per frame, int64: pixels valid in both, in the first only, in the second only, in neither; the sum over the both-valid pixels of
// llrint(min(|a - b| / b, 16) 2^24) (SCALE 2^24, CLAMP 16: at most 2^28 per pixel, 2^59 over 2^31 pixels); and per tolerance k
// the both-valid pixels with |a - b| <= tol_k b, all fp32.  Integer adds: the same words on every run.  error_map (nullable):
// |a - b| / b unclamped, NaN where not both are valid.
//
// No waiting: every loop is bounded by a box or by the list length read once, atomics are single instructions that are never
// retried, no lane, wave or workgroup waits on another.
namespace lrf {

constexpr int RS_NT = 256;
constexpr int RS_SMALL_MAX = 256;                                   // DESIGN.md 4s holds the sweep behind it
constexpr int RS_LARGE_WGS = 1024;                                  // k_rs_large: 4096 wavefronts stride the list ...
constexpr int RS_LARGE_SLICES = 8;                                  // ... in each of 8 grid rows, which share every entry's box
constexpr unsigned long long RS_EMPTY = ~0ull;
constexpr int AG_NT = 256;
constexpr int AG_PX = 8;                                            // pixels per lane
constexpr int AG_WORDS = 16;                                        // int64 per frame: both, first, second, neither, sum, 3 x 0, within[8]
constexpr float AG_CLAMP = 16.0f;
constexpr double AG_SCALE = 16777216.0;                             // 2^24

struct RasterArgs {
  const float* vertices; const uint8_t* rgb8; const int* faces; const float* c2w; const float* focal; const float* center;
  int Nv, Nf, V, H, W, cull;
  float d_min, d_max;
  int small_max;
};

// step 1 -> 0: q holds the camera-space corners; 1: an index outside [0, Nv); 2: two equal indices; 3: a coordinate not finite
__device__ __forceinline__ int rs_face(const RasterArgs& a, int v, int f, float (&q)[3][3], int (&idx)[3]) {
  const int kind = sm_face(a.faces, f, a.Nv, &idx[0], &idx[1], &idx[2]);
  if (kind) return kind;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[c] = a.vertices[3 * (size_t)idx[k] + c];
      finite = finite && (__float_as_uint(p[c]) & 0x7FFFFFFFu) < 0x7F800000u;
    }
    to_camera(a.c2w + (size_t)v * 12, p, q[k]);
  }
  return finite ? 0 : 3;
}

__device__ __forceinline__ int rs_lo(float a, int n) {              // NaN -> 0
  a = floorf(a) - 1.0f;
  return a > 0.0f ? (a < (float)n ? (int)a : n) : 0;
}
__device__ __forceinline__ int rs_hi(float b, int n) {              // NaN -> n - 1
  b = ceilf(b) + 1.0f;
  return b < (float)(n - 1) ? (b >= 0.0f ? (int)b : -1) : n - 1;
}

// the conservative pixel box [i0, i1] x [j0, j1] of a face; false when the face is skipped or the box is empty
__device__ __forceinline__ bool rs_box(const float (&q)[3][3], float f, float cx, float cy, int W, int H, int& i0, int& i1, int& j0,
                                       int& j1) {
#pragma clang fp contract(off)
  const float n0 = -q[0][2], n1 = -q[1][2], n2 = -q[2][2];
  if (n0 <= 0.0f && n1 <= 0.0f && n2 <= 0.0f) return false;
  i0 = 0; i1 = W - 1; j0 = 0; j1 = H - 1;
  if (n0 > 0.0f && n1 > 0.0f && n2 > 0.0f) {
    float u[3], w[3];
    bool num = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float nz = -q[k][2];
      u[k] = q[k][0] / nz * f + cx - 0.5f;
      w[k] = -q[k][1] / nz * f + cy - 0.5f;
      num = num && u[k] == u[k] && w[k] == w[k];
    }
    if (num) {
      i0 = rs_lo(fminf(fminf(u[0], u[1]), u[2]), W); i1 = rs_hi(fmaxf(fmaxf(u[0], u[1]), u[2]), W);
      j0 = rs_lo(fminf(fminf(w[0], w[1]), w[2]), H); j1 = rs_hi(fmaxf(fmaxf(w[0], w[1]), w[2]), H);
    }
  }
  return i0 <= i1 && j0 <= j1;
}

__device__ __forceinline__ int rs_sign(double U, float axb, float ayb, float axc, float ayc) {
  if (U > 0.0) return 1;
  if (U < 0.0) return -1;
  if (ayb > ayc) return 1;
  if (ayb < ayc) return -1;
  if (axc > axb) return 1;
  if (axc < axb) return -1;
  return 0;
}

// step 2: the ray (x, y, -1) against the face with camera-space corners q -> covered; s the common sign, U the edge functions
__device__ __forceinline__ bool rs_cover(const float (&q)[3][3], float x, float y, int& s, double (&U)[3]) {
#pragma clang fp contract(off)
  float ax[3], ay[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ax[k] = q[k][0] + q[k][2] * x;
    ay[k] = q[k][1] + q[k][2] * y;
  }
  U[0] = (double)ax[1] * (double)ay[2] - (double)ay[1] * (double)ax[2];
  U[1] = (double)ax[2] * (double)ay[0] - (double)ay[2] * (double)ax[0];
  U[2] = (double)ax[0] * (double)ay[1] - (double)ay[0] * (double)ax[1];
  s = rs_sign(U[0], ax[1], ay[1], ax[2], ay[2]);
  const int s1 = rs_sign(U[1], ax[2], ay[2], ax[0], ay[0]);
  const int s2 = rs_sign(U[2], ax[0], ay[0], ax[1], ay[1]);
  return s != 0 && s == s1 && s == s2;
}

// step 3
__device__ __forceinline__ float rs_depth(const float (&q)[3][3], const double (&U)[3]) {
#pragma clang fp contract(off)
  const double n0 = (double)(-q[0][2]), n1 = (double)(-q[1][2]), n2 = (double)(-q[2][2]);
  const double t = ((U[0] * n0 + U[1] * n1) + U[2] * n2) / ((U[0] + U[1]) + U[2]);
  return (float)t;
}

// steps 2 to 4 for one pixel of one (frame, face)
__device__ __forceinline__ void rs_pixel(const RasterArgs& a, const float (&q)[3][3], int v, int f, int i, int j, float x, float y,
                                         unsigned long long* __restrict__ keys, int* __restrict__ crossings) {
  int s;
  double U[3];
  if (!rs_cover(q, x, y, s, U)) return;
  const float t = rs_depth(q, U);
  if (!(pts_finite_pos(t) && t >= a.d_min && t <= a.d_max)) return;
  const size_t p = ((size_t)v * a.H + j) * a.W + i;
  if (crossings) atomicAdd(&crossings[p], 1);
  if ((a.cull == 1 && s < 0) || (a.cull == 2 && s > 0)) return;
  atomicMin(&keys[p], ((unsigned long long)__float_as_uint(t) << 32) | (unsigned long long)(unsigned)f);
}

// keys = all ones, crossings = 0, the list cursor = 0, info = 0
__global__ __launch_bounds__(RS_NT) void k_rs_init(unsigned long long* __restrict__ keys, int* __restrict__ crossings, long long n,
                                                   int* __restrict__ cursor, unsigned long long* __restrict__ info) {
  const long long i = (long long)blockIdx.x * RS_NT + threadIdx.x;
  if (i < n) {
    keys[i] = RS_EMPTY;
    if (crossings) crossings[i] = 0;
  }
  if (i < 4) info[i] = 0ull;
  if (i == 4) *cursor = 0;
}

__global__ __launch_bounds__(RS_NT) void k_rs_faces(RasterArgs a, unsigned long long* __restrict__ keys, int* __restrict__ crossings,
                                                    int* __restrict__ cursor, int2* __restrict__ list,
                                                    unsigned long long* __restrict__ info) {
  const long long g = (long long)blockIdx.x * RS_NT + threadIdx.x;
  int kind = -1, v = 0, f = 0, idx[3];
  float q[3][3];
  if (g < (long long)a.V * a.Nf) {
    v = (int)(g / a.Nf);
    f = (int)(g - (long long)v * a.Nf);
    kind = rs_face(a, v, f, q, idx);
  }
  const bool first = v == 0;
  wave_count(&info[0], first && kind == 1);
  wave_count(&info[1], first && kind == 2);
  wave_count(&info[2], first && kind == 3);
  const float fo = a.focal[0], cx = a.center[0], cy = a.center[1];
  int i0 = 0, i1 = -1, j0 = 0, j1 = -1;
  const bool boxed = kind == 0 && rs_box(q, fo, cx, cy, a.W, a.H, i0, i1, j0, j1);
  const bool large = boxed && (long long)(i1 - i0 + 1) * (j1 - j0 + 1) > a.small_max;
  const unsigned long long lb = __ballot(large);                    // one returning atomicAdd per wave claims its entries
  if (lb) {
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)lb) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(cursor, __popcll(lb));     // at most V Nf entries in all: one per lane of this grid
    base = __shfl(base, leader, 64);
    if (large) list[base + __popcll(lb & ((1ull << lane) - 1ull))] = make_int2(v, f);
  }
  if (!boxed || large) return;
  for (int j = j0; j <= j1; ++j) {
    const float y = pinhole_y((float)j, fo, cy);
    for (int i = i0; i <= i1; ++i) rs_pixel(a, q, v, f, i, j, pinhole_x((float)i, fo, cx), y, keys, crossings);
  }
}

__global__ __launch_bounds__(RS_NT) void k_rs_large(RasterArgs a, unsigned long long* __restrict__ keys, int* __restrict__ crossings,
                                                    const int* __restrict__ cursor, const int2* __restrict__ list) {
  const int lane = threadIdx.x & 63;
  const int n = *cursor;
  const int waves = gridDim.x * (RS_NT / 64);
  const float fo = a.focal[0], cx = a.center[0], cy = a.center[1];
  for (int e = blockIdx.x * (RS_NT / 64) + (threadIdx.x >> 6); e < n; e += waves) {
    const int2 vf = list[e];
    float q[3][3];
    int idx[3], i0, i1, j0, j1;
    if (rs_face(a, vf.x, vf.y, q, idx) != 0) continue;              // cannot happen: k_rs_faces listed a valid face
    if (!rs_box(q, fo, cx, cy, a.W, a.H, i0, i1, j0, j1)) continue;
    const int bw = i1 - i0 + 1, npx = bw * (j1 - j0 + 1);           // <= H W < 2^31
    for (int p = blockIdx.y * 64 + lane; p < npx; p += 64 * gridDim.y) {   // this slice's 64-pixel groups of the box
      const int r = p / bw;
      const int i = i0 + (p - r * bw), j = j0 + r;
      rs_pixel(a, q, vf.x, vf.y, i, j, pinhole_x((float)i, fo, cx), pinhole_y((float)j, fo, cy), keys, crossings);
    }
  }
}

__global__ __launch_bounds__(RS_NT) void k_rs_resolve(RasterArgs a, const unsigned long long* __restrict__ keys,
                                                      float* __restrict__ depth, int* __restrict__ face, uint8_t* __restrict__ rgb8_out,
                                                      float* __restrict__ weights) {
#pragma clang fp contract(off)
  const long long p = (long long)blockIdx.x * RS_NT + threadIdx.x;
  if (p >= (long long)a.V * a.H * a.W) return;
  const unsigned long long key = keys[p];
  const bool hit = key != RS_EMPTY;
  const int f = hit ? (int)(unsigned)(key & 0xFFFFFFFFull) : -1;
  depth[p] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
  face[p] = f;
  if (!rgb8_out && !weights) return;
  float wf[3] = {0.0f, 0.0f, 0.0f};
  float col[3] = {0.0f, 0.0f, 0.0f};
  if (hit) {
    const int hw = a.H * a.W;
    const int v = (int)(p / hw);
    const int r = (int)(p - (long long)v * hw);
    const int j = r / a.W, i = r - j * a.W;
    float q[3][3];
    int idx[3], s;
    double U[3];
    rs_face(a, v, f, q, idx);                                       // a winner is a valid face
    rs_cover(q, pinhole_x((float)i, a.focal[0], a.center[0]), pinhole_y((float)j, a.focal[0], a.center[1]), s, U);
    const double D = (U[0] + U[1]) + U[2];
    const double w0 = U[0] / D, w1 = U[1] / D, w2 = U[2] / D;
    wf[0] = (float)w0; wf[1] = (float)w1; wf[2] = (float)w2;
    if (rgb8_out) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double c0 = (double)a.rgb8[3 * (size_t)idx[0] + c], c1 = (double)a.rgb8[3 * (size_t)idx[1] + c],
                     c2 = (double)a.rgb8[3 * (size_t)idx[2] + c];
        const double m = rint((w0 * c0 + w1 * c1) + w2 * c2);
        col[c] = (float)(m < 0.0 ? 0.0 : (m > 255.0 ? 255.0 : m));
      }
    }
  }
  if (weights) { weights[3 * p] = wf[0]; weights[3 * p + 1] = wf[1]; weights[3 * p + 2] = wf[2]; }
  if (rgb8_out) { rgb8_out[3 * p] = (uint8_t)col[0]; rgb8_out[3 * p + 1] = (uint8_t)col[1]; rgb8_out[3 * p + 2] = (uint8_t)col[2]; }
}

struct AgreeArgs {
  const float* a; const float* b;
  int V, H, W, n_tol;
  float tol[LRF_AGREEMENT_MAX_TOLS];
  float d_min, d_max;
};

__global__ __launch_bounds__(RS_NT) void k_ag_zero(unsigned long long* __restrict__ counts, long long n) {
  const long long i = (long long)blockIdx.x * RS_NT + threadIdx.x;
  if (i < n) counts[i] = 0ull;
}

// blockIdx.y: the frame; blockIdx.x: AG_NT AG_PX consecutive pixels of it
__global__ __launch_bounds__(AG_NT) void k_depth_agreement(AgreeArgs g, unsigned long long* __restrict__ counts,
                                                           float* __restrict__ error_map) {
#pragma clang fp contract(off)
  const int hw = g.H * g.W;
  const int v = blockIdx.y;
  const size_t base = (size_t)v * hw;
  unsigned n_both = 0, n_a = 0, n_b = 0, n_none = 0, within[LRF_AGREEMENT_MAX_TOLS];
  unsigned long long sum = 0;
#pragma unroll
  for (int k = 0; k < LRF_AGREEMENT_MAX_TOLS; ++k) within[k] = 0;
#pragma unroll
  for (int k = 0; k < AG_PX; ++k) {
    const long long p = ((long long)blockIdx.x * AG_PX + k) * AG_NT + threadIdx.x;
    if (p >= hw) continue;
    const float da = g.a[base + p], db = g.b[base + p];
    const bool va = pts_finite_pos(da) && da >= g.d_min && da <= g.d_max;
    const bool vb = pts_finite_pos(db) && db >= g.d_min && db <= g.d_max;
    float rel = __uint_as_float(0x7FC00000u);
    if (va && vb) {
      const float diff = fabsf(da - db);
      rel = diff / db;
      ++n_both;
      sum += (unsigned long long)llrint((double)fminf(rel, AG_CLAMP) * AG_SCALE);
#pragma unroll
      for (int t = 0; t < LRF_AGREEMENT_MAX_TOLS; ++t)
        if (t < g.n_tol && diff <= g.tol[t] * db) ++within[t];
    } else if (va) ++n_a;
    else if (vb) ++n_b;
    else ++n_none;
    if (error_map) error_map[base + p] = rel;
  }
  n_both = wave_sum(n_both); n_a = wave_sum(n_a); n_b = wave_sum(n_b);
  n_none = wave_sum(n_none); sum = wave_sum(sum);
#pragma unroll
  for (int t = 0; t < LRF_AGREEMENT_MAX_TOLS; ++t) within[t] = wave_sum(within[t]);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* c = counts + (size_t)v * AG_WORDS;
    if (n_both) atomicAdd(&c[0], (unsigned long long)n_both);
    if (n_a) atomicAdd(&c[1], (unsigned long long)n_a);
    if (n_b) atomicAdd(&c[2], (unsigned long long)n_b);
    if (n_none) atomicAdd(&c[3], (unsigned long long)n_none);
    if (sum) atomicAdd(&c[4], sum);
#pragma unroll
    for (int t = 0; t < LRF_AGREEMENT_MAX_TOLS; ++t)
      if (within[t]) atomicAdd(&c[8 + t], (unsigned long long)within[t]);
  }
}

// true when lrf_mesh_rasterize takes the shape
static bool raster_shape(long long V, long long H, long long W, long long Nf) {
  return V >= 1 && H >= 1 && W >= 1 && Nf >= 0 && V * H * W < (1ll << 31) && Nf < (1ll << 31) && V * Nf < (1ll << 31);
}

// the workspace: a key per pixel, the list of large (frame, face) pairs, its cursor (8 bytes)
struct RasterWs { unsigned long long* keys; int2* list; int* cursor; size_t bytes; };
static RasterWs raster_carve(void* workspace, long long n_px, long long n_pairs) {
  Carver c(workspace);
  RasterWs w;
  w.keys = c.take<unsigned long long>((size_t)n_px);
  w.list = c.take<int2>((size_t)n_pairs);
  w.cursor = c.take<int>(2);
  w.bytes = c.bytes();
  return w;
}

static int raster_run(const char* who, const LrfMeshRaster* m, float* depth, int32_t* face, uint8_t* rgb8_out, float* weights,
                      int32_t* crossings, int64_t* info, void* workspace, int small_max, void* stream) {
  if (!m) return refuse(who, "null argument");
  if (!raster_shape(m->V, m->H, m->W, m->Nf) || m->Nv < 0 || m->Nv >= (1ll << 31) || (m->Nf > 0 && m->Nv < 1))
    return refuse(who, "need V, H, W >= 1, V H W < 2^31, 0 <= Nv < 2^31, 0 <= Nf, V Nf < 2^31 and vertices for the faces");
  if (!m->cam2world || !m->focal || !m->center || !depth || !face || !info || !workspace) return refuse(who, "null argument");
  if (m->Nf > 0 && (!m->vertices || !m->faces)) return refuse(who, "null argument");
  if (!m->rgb8 != !rgb8_out) return refuse(who, "rgb8 and rgb8_out go together");
  if (m->cull < 0 || m->cull > 2) return refuse(who, "cull must be 0 (none), 1 (back) or 2 (front)");
  if (!(m->d_min <= m->d_max)) return refuse(who, "need d_min <= d_max");
  if (small_max < 0) return refuse(who, "small_max must be >= 0");
  if (misaligned(3, m->vertices, m->faces, m->cam2world, m->focal, m->center, depth, face, weights, crossings))
    return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, info, workspace)) return refuse(who, "info and workspace must be 8-byte aligned");
  RasterArgs a;
  memset(&a, 0, sizeof(a));
  a.vertices = m->vertices; a.rgb8 = m->rgb8; a.faces = m->faces; a.c2w = m->cam2world; a.focal = m->focal; a.center = m->center;
  a.Nv = (int)m->Nv; a.Nf = (int)m->Nf; a.V = m->V; a.H = m->H; a.W = m->W; a.cull = m->cull;
  a.d_min = m->d_min; a.d_max = m->d_max; a.small_max = small_max;
  const long long n_px = (long long)m->V * m->H * m->W, n_pairs = (long long)m->V * m->Nf;
  const RasterWs w = raster_carve(workspace, n_px, n_pairs);
  unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_rs_init, blocks_for(n_px, RS_NT), RS_NT, st, w.keys, crossings, n_px, w.cursor, inf));
  if (n_pairs) {
    LRF_TRY(launch(k_rs_faces, blocks_for(n_pairs, RS_NT), RS_NT, st, a, w.keys, crossings, w.cursor, w.list, inf));
    const unsigned wgs = std::min<unsigned>(RS_LARGE_WGS, blocks_for(n_pairs, RS_NT / 64));
    LRF_TRY(launch(k_rs_large, dim3(wgs, RS_LARGE_SLICES), RS_NT, st, a, w.keys, crossings, w.cursor, w.list));
  }
  return launch(k_rs_resolve, blocks_for(n_px, RS_NT), RS_NT, st, a, w.keys, depth, face, rgb8_out, weights);
}

}  // namespace lrf

extern "C" size_t lrf_mesh_rasterize_workspace_bytes(int32_t V, int32_t H, int32_t W, int64_t Nf) {
  using namespace lrf;
  return raster_shape(V, H, W, Nf) ? raster_carve(nullptr, (long long)V * H * W, V * Nf).bytes : 0;
}

extern "C" int lrf_mesh_rasterize(const LrfMeshRaster* m, float* depth, int32_t* face, uint8_t* rgb8_out, float* weights,
                                  int32_t* crossings, int64_t* info, void* workspace, void* stream) {
  return lrf::raster_run("lrf_mesh_rasterize", m, depth, face, rgb8_out, weights, crossings, info, workspace, lrf::RS_SMALL_MAX, stream);
}

extern "C" int lrf_debug_mesh_rasterize(const LrfMeshRaster* m, float* depth, int32_t* face, uint8_t* rgb8_out, float* weights,
                                        int32_t* crossings, int64_t* info, void* workspace, int32_t small_max, void* stream) {
  return lrf::raster_run("lrf_debug_mesh_rasterize", m, depth, face, rgb8_out, weights, crossings, info, workspace, small_max, stream);
}

extern "C" int lrf_depth_agreement(const float* mesh_depth, const float* depth, int32_t V, int32_t H, int32_t W, const float* rel_tols,
                                   int32_t n_tols, float d_min, float d_max, int64_t* counts, float* error_map, void* stream) {
  using namespace lrf;
  if (V < 1 || V > 65535 || H < 1 || W < 1 || (long long)V * H * W >= (1ll << 31))
    return set_err("lrf_depth_agreement: need 1 <= V <= 65535, H, W >= 1 and V H W < 2^31");
  if (n_tols < 0 || n_tols > LRF_AGREEMENT_MAX_TOLS) return set_err("lrf_depth_agreement: n_tols must lie in [0, LRF_AGREEMENT_MAX_TOLS]");
  if (!mesh_depth || !depth || !counts || (n_tols && !rel_tols)) return set_err("lrf_depth_agreement: null argument");
  if (!(d_min <= d_max)) return set_err("lrf_depth_agreement: need d_min <= d_max");
  for (int k = 0; k < n_tols; ++k)
    if (!(rel_tols[k] >= 0.0f)) return set_err("lrf_depth_agreement: a tolerance must be >= 0");
  if (misaligned(3, mesh_depth, depth, error_map)) return set_err("lrf_depth_agreement: float arrays must be 4-byte aligned");
  if (misaligned(7, counts)) return set_err("lrf_depth_agreement: counts must be 8-byte aligned");
  AgreeArgs g;
  memset(&g, 0, sizeof(g));
  g.a = mesh_depth; g.b = depth; g.V = V; g.H = H; g.W = W; g.n_tol = n_tols; g.d_min = d_min; g.d_max = d_max;
  for (int k = 0; k < n_tols; ++k) g.tol[k] = rel_tols[k];
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  const long long words = (long long)V * AG_WORDS;
  LRF_TRY(launch(k_ag_zero, blocks_for(words, RS_NT), RS_NT, st, c, words));
  return launch(k_depth_agreement, dim3(blocks_for((long long)H * W, AG_NT * AG_PX), (unsigned)V), AG_NT, st, g, c, error_map);
}
