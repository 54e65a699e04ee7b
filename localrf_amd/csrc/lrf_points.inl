// lrf_points.inl -- rendered depth fused into ONE filtered, ordered, coloured world-space point list (included by
// lrf_render.hip; the scan is lrf_compact.inl's, the host helpers lrf_host.inl's).  V depth images [V,H,W] with their camera-to-world
// matrices go in; the points of the kept pixels come out in (frame, row, column) order, the same list on every run and for
// every launch geometry.
//
// A candidate is a pixel (i, j) of frame v with i % stride == 0 and j % stride == 0; candidates are numbered in (frame, row,
// column) order.  Per candidate, in fp32 with contraction off so that a numpy restatement matches bit for bit:
//   1. d = depth[v,j,i]; dropped unless finite, positive and d_min <= d <= d_max;
//   2. dir = pixel_dir(...) (lrf_scene.inl: ids2pixel + get_ray_directions_lean / _360; z = -1 for a pinhole, so the depth
//      is a multiple of the UN-normalised direction, tensorBase.py:615); pc = dir * d; pw = R_v pc + t_v, row by row as
//      ((r0 x + r1 y) + r2 z) + t;
//   3. consistency (pinhole only), for every offset o with n = v + o in [0, V): q = R_n^T (pw - t_n), column by column as
//      (c0 dx + c1 dy) + c2 dz; fails behind the camera (-q.z <= 0); (u, w) = (q.x / -q.z * f + cx - 0.5,
//      -q.y / -q.z * f + cy - 0.5) (utils/utils.py:15-21 without the in-place clip); iu = rint(u), iw = rint(w), ties to even;
//      fails outside the image; dn = depth[n,iw,iu] must be finite and positive; passes when |-q.z - dn| <= rel_tol * dn.
//      Kept when passes >= min(min_consistent, offsets that stayed in range).
//
// Ordered compaction in two passes and a scan:
//   k_points_mark   one lane per candidate, 64 consecutive candidates per wave and step (consecutive columns of a row: the
//                   depth loads coalesce at stride 1, the neighbour gathers land on nearby lines).  The wave's ballot is the
//                   keep word of its 64 candidates, stored by one lane; a workgroup covers PTS_WORDS_WG words and leaves
//                   their popcount.
//   k_points_scan   (lrf_compact.inl) ONE workgroup turns the workgroup counts into exclusive bases in place and leaves the
//                   total in count[0].
//   k_points_write  reads the keep words, recomputes pw of the kept candidates with the same instructions and writes row
//                   base + popcount(word & lanes_below).  Rows at or beyond `capacity` are not written; count[0] is the
//                   true total.
// Cited lines are relative to the reference's localTensoRF directory.
namespace lrf {

constexpr int PTS_NT = 256;
constexpr int PTS_WORDS_WAVE = 4;                                   // 64-candidate steps per wave
constexpr int PTS_WORDS_WG = (PTS_NT / 64) * PTS_WORDS_WAVE;        // keep words per workgroup
constexpr int PTS_CAND_WG = 64 * PTS_WORDS_WG;                      // candidates per workgroup

struct PointsArgs {
  const float* depth; const uint8_t* rgb8; const float* c2w; const float* focal; const float* center;
  int V, H, W, fov360, stride;
  int Hs, Ws, n_cand;                                               // candidate grid per frame; V Hs Ws
  float d_min, d_max;
  int n_neigh, neigh[LRF_POINTS_MAX_NEIGH];
  float rel_tol;
  int min_consistent;
};

__device__ __forceinline__ bool pts_finite_pos(float d) {
  return (__float_as_uint(d) & 0x7FFFFFFFu) < 0x7F800000u && d > 0.0f;
}

// step 2's arithmetic, shared with the block touch (lrf_tsdf_blocks.inl): the world point at `depth` along the pixel's direction
// under the camera M [3,4] (camera-to-world)
__device__ __forceinline__ void world_point(const float* __restrict__ M, const PixDir& p, float depth, float (&pw)[3]) {
#pragma clang fp contract(off)
  const float x = p.x * depth, y = p.y * depth, z = p.z * depth;
  pw[0] = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  pw[1] = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  pw[2] = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
}

// candidate c -> frame v, pixel id pix; false when its depth fails step 1, else pw = the world point
__device__ __forceinline__ bool pts_world(const PointsArgs& a, int c, float f, float cx, float cy, int& v, int& pix,
                                          float (&pw)[3]) {
#pragma clang fp contract(off)
  const int per = a.Hs * a.Ws;
  v = c / per;
  const int r = c - v * per;
  const int js = r / a.Ws, is = r - js * a.Ws;
  pix = js * a.stride * a.W + is * a.stride;
  const float d = a.depth[(size_t)v * a.H * a.W + pix];
  if (!(pts_finite_pos(d) && d >= a.d_min && d <= a.d_max)) return false;
  world_point(a.c2w + (size_t)v * 12, pixel_dir(pix, a.W, a.H, a.fov360, f, cx, cy), d, pw);
  return true;
}

// the first half of step 3, shared with the mesh rasteriser (lrf_mesh_raster.inl): world point pw into the frame of the camera
// M [3,4] (camera-to-world): d = pw - t, q = R^T d column by column as (c0 dx + c1 dy) + c2 dz
__device__ __forceinline__ void to_camera(const float* __restrict__ M, const float (&pw)[3], float (&q)[3]) {
#pragma clang fp contract(off)
  const float dx = pw[0] - M[3], dy = pw[1] - M[7], dz = pw[2] - M[11];
  q[0] = (M[0] * dx + M[4] * dy) + M[8] * dz;
  q[1] = (M[1] * dx + M[5] * dy) + M[9] * dz;
  q[2] = (M[2] * dx + M[6] * dy) + M[10] * dz;
}

// step 3's projection, shared with the TSDF integration (lrf_mesh.inl): world point pw into the camera M [3,4] (camera-to-world)
// of an H x W pinhole image.  false behind the camera (nz = -q.z <= 0) or outside the image; else nz and the nearest pixel
// (iu, iw), ties to even.
__device__ __forceinline__ bool reproject(const float* __restrict__ M, const float (&pw)[3], float f, float cx, float cy, int W,
                                          int H, float& nz, int& iu, int& iw) {
#pragma clang fp contract(off)
  float q[3];
  to_camera(M, pw, q);
  const float qx = q[0], qy = q[1], qz = q[2];
  nz = -qz;
  if (!(nz > 0.0f)) return false;
  const float u = qx / nz * f + cx - 0.5f;
  const float w = -qy / nz * f + cy - 0.5f;
  const float ru = rintf(u), rw = rintf(w);
  if (!(ru >= 0.0f && ru < 2147483648.0f && rw >= 0.0f && rw < 2147483648.0f)) return false;   // NaN fails
  iu = (int)ru; iw = (int)rw;
  return iu < W && iw < H;
}

__device__ __forceinline__ bool pts_consistent(const PointsArgs& a, int v, const float (&pw)[3], float f, float cx, float cy) {
#pragma clang fp contract(off)
  int in_range = 0, pass = 0;
  for (int k = 0; k < a.n_neigh; ++k) {
    const long long nl = (long long)v + a.neigh[k];
    if (nl < 0 || nl >= a.V) continue;                              // counts neither for nor against
    ++in_range;
    float nz;
    int iu, iw;
    if (!reproject(a.c2w + (size_t)nl * 12, pw, f, cx, cy, a.W, a.H, nz, iu, iw)) continue;
    const float dn = a.depth[(size_t)nl * a.H * a.W + (size_t)iw * a.W + iu];
    if (!pts_finite_pos(dn)) continue;
    if (fabsf(nz - dn) <= a.rel_tol * dn) ++pass;
  }
  return pass >= min(a.min_consistent, in_range);
}

__global__ __launch_bounds__(PTS_NT) void k_points_mark(PointsArgs a, unsigned long long* __restrict__ bits,
                                                        unsigned* __restrict__ wg) {
  __shared__ unsigned red[PTS_NT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float f = a.fov360 ? 1.0f : a.focal[0];
  const float cx = a.fov360 ? 0.0f : a.center[0], cy = a.fov360 ? 0.0f : a.center[1];
  unsigned cnt = 0;
  for (int k = 0; k < PTS_WORDS_WAVE; ++k) {
    const long long word = (long long)blockIdx.x * PTS_WORDS_WG + wv * PTS_WORDS_WAVE + k;
    const long long c = word * 64 + lane;
    bool keep = false;
    if (c < a.n_cand) {
      int v, pix;
      float pw[3];
      if (pts_world(a, (int)c, f, cx, cy, v, pix, pw)) keep = a.n_neigh == 0 || pts_consistent(a, v, pw, f, cx, cy);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) bits[word] = m;                                  // every word of the workspace is written
    cnt += (unsigned)__popcll(m);
  }
  unsigned s[1] = {cnt};                                            // every lane of a wave holds the wave's count already
  block_fold<PTS_NT, false>(s, red, OpSum());
  if (threadIdx.x == 0) wg[blockIdx.x] = s[0];
}

__global__ __launch_bounds__(PTS_NT) void k_points_write(PointsArgs a, const unsigned long long* __restrict__ bits,
                                                         const unsigned* __restrict__ wg, long long capacity,
                                                         float* __restrict__ xyz, uint8_t* __restrict__ rgb8_out,
                                                         int* __restrict__ src) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float f = a.fov360 ? 1.0f : a.focal[0];
  const float cx = a.fov360 ? 0.0f : a.center[0], cy = a.fov360 ? 0.0f : a.center[1];
  const long long word0 = (long long)blockIdx.x * PTS_WORDS_WG;
  long long run = wg[blockIdx.x];
  for (int i = 0; i < wv * PTS_WORDS_WAVE; ++i) run += __popcll(bits[word0 + i]);
  for (int k = 0; k < PTS_WORDS_WAVE; ++k) {
    const long long word = word0 + wv * PTS_WORDS_WAVE + k;
    const unsigned long long m = bits[word];
    const long long row = run + __popcll(m & ((1ull << lane) - 1ull));
    run += __popcll(m);
    if (!((m >> lane) & 1ull) || row >= capacity) continue;
    int v, pix;
    float pw[3];
    pts_world(a, (int)(word * 64 + lane), f, cx, cy, v, pix, pw);   // a set bit: the candidate exists and passed step 1
    xyz[3 * row + 0] = pw[0]; xyz[3 * row + 1] = pw[1]; xyz[3 * row + 2] = pw[2];
    src[2 * row + 0] = v; src[2 * row + 1] = pix;
    if (rgb8_out) {
      const uint8_t* c = a.rgb8 + 3 * ((size_t)v * a.H * a.W + pix);
      rgb8_out[3 * row + 0] = c[0]; rgb8_out[3 * row + 1] = c[1]; rgb8_out[3 * row + 2] = c[2];
    }
  }
}

// candidates of a shape, or 0 when lrf_points_fuse refuses it
static long long points_candidates(int V, int H, int W, int stride) {
  if (V < 1 || H < 1 || W < 1 || stride < 1 || (long long)V * H * W >= (1ll << 31)) return 0;
  return (long long)V * ((H + stride - 1) / stride) * ((W + stride - 1) / stride);
}

// the workspace of n candidates: the keep words, then the workgroup counts
struct PointsWs { int n_wg; unsigned long long* bits; unsigned* wg; size_t bytes; };
static PointsWs points_carve(void* workspace, long long n) {
  Carver c(workspace);
  PointsWs w;
  w.n_wg = (int)blocks_for(n, PTS_CAND_WG);
  w.bits = c.take<unsigned long long>((size_t)w.n_wg * PTS_WORDS_WG);
  w.wg = c.take<unsigned>(w.n_wg);
  w.bytes = c.bytes();
  return w;
}

}  // namespace lrf

extern "C" size_t lrf_points_workspace_bytes(int32_t V, int32_t H, int32_t W, int32_t stride) {
  using namespace lrf;
  const long long n = points_candidates(V, H, W, stride);
  return n ? points_carve(nullptr, n).bytes : 0;
}

extern "C" int lrf_points_fuse(const LrfPointsFuse* p, int64_t capacity, float* xyz, uint8_t* rgb8_out, int32_t* src,
                               int64_t* count, void* workspace, void* stream) {
  using namespace lrf;
  if (!p) return set_err("lrf_points_fuse: null argument");
  const long long n = points_candidates(p->V, p->H, p->W, p->stride);
  if (!n) return set_err("lrf_points_fuse: need V, H, W, stride >= 1 and V H W < 2^31");
  if (!p->depth || !p->cam2world || !xyz || !src || !count || !workspace) return set_err("lrf_points_fuse: null argument");
  if (!p->rgb8 != !rgb8_out) return set_err("lrf_points_fuse: rgb8 and rgb8_out go together");
  if (!p->fov360 && (!p->focal || !p->center)) return set_err("lrf_points_fuse: pinhole cameras need focal and center");
  if (capacity < 0) return set_err("lrf_points_fuse: capacity must be >= 0");
  if (!(p->d_min <= p->d_max)) return set_err("lrf_points_fuse: need d_min <= d_max");
  if (p->n_neigh < 0 || p->n_neigh > LRF_POINTS_MAX_NEIGH) return set_err("lrf_points_fuse: n_neigh must lie in [0, LRF_POINTS_MAX_NEIGH]");
  if (p->n_neigh && p->fov360) return set_err("lrf_points_fuse: the consistency test needs a pinhole camera (no reprojection at 360 degrees)");
  for (int i = 0; i < p->n_neigh; ++i) {
    if (p->neigh[i] == 0) return set_err("lrf_points_fuse: a neighbour offset must not be 0");
    for (int j = 0; j < i; ++j)
      if (p->neigh[j] == p->neigh[i]) return set_err("lrf_points_fuse: repeated neighbour offset");
  }
  if (p->n_neigh && !(p->rel_tol >= 0.0f)) return set_err("lrf_points_fuse: rel_tol must be >= 0");
  if (p->n_neigh && p->min_consistent < 0) return set_err("lrf_points_fuse: min_consistent must be >= 0");
  if (misaligned(3, p->depth, p->cam2world, p->focal, p->center, xyz, src))
    return set_err("lrf_points_fuse: float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, count, workspace)) return set_err("lrf_points_fuse: count and workspace must be 8-byte aligned");
  PointsArgs a;
  memset(&a, 0, sizeof(a));
  a.depth = p->depth; a.rgb8 = p->rgb8; a.c2w = p->cam2world; a.focal = p->focal; a.center = p->center;
  a.V = p->V; a.H = p->H; a.W = p->W; a.fov360 = p->fov360 ? 1 : 0; a.stride = p->stride;
  a.Hs = (p->H + p->stride - 1) / p->stride; a.Ws = (p->W + p->stride - 1) / p->stride;
  a.n_cand = (int)n;
  a.d_min = p->d_min; a.d_max = p->d_max;
  a.n_neigh = p->n_neigh;
  for (int i = 0; i < p->n_neigh; ++i) a.neigh[i] = p->neigh[i];
  a.rel_tol = p->rel_tol; a.min_consistent = p->min_consistent;
  const PointsWs w = points_carve(workspace, n);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_points_mark, w.n_wg, PTS_NT, st, a, w.bits, w.wg));
  LRF_TRY(launch(k_points_scan, 1, PTS_SCAN_NT, st, w.wg, w.n_wg, reinterpret_cast<long long*>(count)));
  LRF_TRY(launch(k_points_write, w.n_wg, PTS_NT, st, a, w.bits, w.wg, capacity, xyz, rgb8_out, src));
  return 0;
}
