// lrf_frames.inl -- the device frame store (included by lrf_render.hip): the train split of dataLoader/localrf_dataset.py
// (LocalRFDataset) held on the GPU as a window of `capacity` frame slots, and the three kernels around it.
//
// k_frames_gather (one launch per iteration): the rows of sample() (localrf_dataset.py:303-313, `self.all_X[idx_sample]`
//   for the seven dataset tensors) for V views x n rays.  Row r reads view view_ids[r / n] through the device table
//   slot_of[num_images] (-1: not resident) and pixel ray_ids[r] mod n_px (global ids view * n_px + pix as the reference's
//   `idx`, or per-view pixel ids: both give the same pixel).  A view outside [0, num_images) or without a slot gets NaN rows
//   and sets LRF_FRAMES_ERR_NOT_RESIDENT in the status word (an integer atomic OR): no trap, no host read.  The table and
//   the status word live at fixed addresses and are rewritten with stream-ordered copies, so a captured gather stays valid
//   when the window moves.
// k_decode_flow: decode_flow (utils/utils.py:67-71) times flow_scale (localrf_dataset.py:193-194), into a slot.
// k_frame_sharpness + k_frame_weight: the loss weight of localrf_dataset.py:229-235, var(Laplacian(grey(img))) x motion mask.
namespace lrf {

constexpr int FR_NT = 256;
constexpr int SH_PARTS = 256;        // fixed partition of the sharpness sums: partial k covers pixels k*FR_NT + t + j*SH_PARTS*FR_NT
constexpr int SH_MAX_PX = 1 << 21;   // N S2 and S1^2 stay below 2^63: |Laplacian| <= 4 * 255, so N^2 1020^2 < 2^63 needs N < 2.97e6

__global__ __launch_bounds__(FR_NT) void k_frames_gather(LrfFrameWindow w, const long long* __restrict__ view_ids,
                                                          const long long* __restrict__ ray_ids, int V, int n,
                                                          float* __restrict__ rgbs, float* __restrict__ loss_weights,
                                                          float* __restrict__ invdepths, float* __restrict__ fwd_flow,
                                                          float* __restrict__ fwd_mask, float* __restrict__ bwd_flow,
                                                          float* __restrict__ bwd_mask) {
  const long long i = (long long)blockIdx.x * FR_NT + threadIdx.x;
  if (i >= (long long)V * n) return;
  const long long v = view_ids[i / n];
  int s = -1;
  if (v >= 0 && v < w.num_images) s = w.slot_of[v];
  if (s < 0 || s >= w.capacity) {
    const float nan = __builtin_nanf("");
    if (rgbs) { rgbs[3 * i] = nan; rgbs[3 * i + 1] = nan; rgbs[3 * i + 2] = nan; }
    if (loss_weights) loss_weights[i] = nan;
    if (invdepths) invdepths[i] = nan;
    if (fwd_flow) { fwd_flow[2 * i] = nan; fwd_flow[2 * i + 1] = nan; }
    if (fwd_mask) fwd_mask[i] = nan;
    if (bwd_flow) { bwd_flow[2 * i] = nan; bwd_flow[2 * i + 1] = nan; }
    if (bwd_mask) bwd_mask[i] = nan;
    atomicOr(w.status, (unsigned)LRF_FRAMES_ERR_NOT_RESIDENT);
    return;
  }
  long long px = ray_ids[i] % w.n_px;
  if (px < 0) px += w.n_px;                                   // (ids are non-negative in the reference; a floored mod regardless)
  const size_t q = (size_t)s * w.n_px + (size_t)px;
  if (rgbs) { rgbs[3 * i] = w.rgb[3 * q]; rgbs[3 * i + 1] = w.rgb[3 * q + 1]; rgbs[3 * i + 2] = w.rgb[3 * q + 2]; }
  if (loss_weights) loss_weights[i] = w.loss_weight[q];
  if (invdepths) invdepths[i] = w.invdepth[q];
  if (fwd_flow) { fwd_flow[2 * i] = w.fwd_flow[2 * q]; fwd_flow[2 * i + 1] = w.fwd_flow[2 * q + 1]; }
  if (fwd_mask) fwd_mask[i] = w.fwd_mask[q];
  if (bwd_flow) { bwd_flow[2 * i] = w.bwd_flow[2 * q]; bwd_flow[2 * i + 1] = w.bwd_flow[2 * q + 1]; }
  if (bwd_mask) bwd_mask[i] = w.bwd_mask[q];
}

// utils.py:67-71: flow = (float32(e) - 2^15) / 2^8 (both steps exact in fp32), mask = e[..., 2] > 2^15; then
// localrf_dataset.py:193-194 multiplies the fp32 array by the Python float flow_scale, which numpy rounds to fp32 first
// (a float32 array times a Python scalar stays float32: tests/test_frames_host.py checks it).  `scale` is that fp32 value.
__global__ __launch_bounds__(FR_NT) void k_decode_flow(const unsigned short* __restrict__ enc, int n_px, float scale,
                                                        float* __restrict__ flow, float* __restrict__ mask) {
  const int i = blockIdx.x * FR_NT + threadIdx.x;
  if (i >= n_px) return;
  const unsigned short e0 = enc[3 * (size_t)i], e1 = enc[3 * (size_t)i + 1], e2 = enc[3 * (size_t)i + 2];
  flow[2 * (size_t)i] = ((float)e0 - 32768.0f) / 256.0f * scale;
  flow[2 * (size_t)i + 1] = ((float)e1 - 32768.0f) / 256.0f * scale;
  mask[i] = e2 > 32768 ? 1.0f : 0.0f;
}

// cv2.cvtColor((img * 255).astype(np.uint8), cv2.COLOR_RGB2GRAY) for one pixel.  img * 255 is an fp32 product and astype
// truncates: the 8-bit values k / 255 come back as k, but a resized image (INTER_AREA averages) holds other values.  Values outside [0, 1] (where numpy's cast is undefined) are clamped.
// The grey conversion is OpenCV's documented fixed-point form for 8-bit images: (4899 R + 9617 G + 1868 B + 8192) >> 14.
// OpenCV is not a dependency, so the tests pin these constants, not OpenCV itself.
__device__ inline int grey_u8(const float* __restrict__ p) {
  int c[3];
  for (int k = 0; k < 3; ++k) {
    float t = p[k] * 255.0f;
    t = t >= 0.0f ? (t <= 255.0f ? t : 255.0f) : 0.0f;       // (NaN -> 0)
    c[k] = (int)t;                                            // truncation toward zero
  }
  return (4899 * c[0] + 9617 * c[1] + 1868 * c[2] + 8192) >> 14;
}
__device__ inline int reflect101(int i, int n) {             // BORDER_REFLECT_101: -1 -> 1, n -> n - 2
  if (n == 1) return 0;
  i = i < 0 ? -i : i;
  return i >= n ? 2 * n - 2 - i : i;
}

// cv2.Laplacian(grey, cv2.CV_32F) (ksize 1: [[0,1,0],[1,-4,1],[0,1,0]]): integer values; each workgroup writes the exact
// int64 sums (S1, S2) of its fixed share of the pixels
__global__ __launch_bounds__(FR_NT) void k_frame_sharpness(const float* __restrict__ rgb, int H, int W, long long* __restrict__ part) {
  __shared__ long long red[2 * (FR_NT / 64)];
  const int tid = threadIdx.x, n_px = H * W;
  long long s[2] = {0, 0};                                     // S1, S2
  for (int i = blockIdx.x * FR_NT + tid; i < n_px; i += SH_PARTS * FR_NT) {
    const int y = i / W, x = i - y * W;
    const int c = grey_u8(rgb + 3 * (size_t)i);
    const int up = grey_u8(rgb + 3 * ((size_t)reflect101(y - 1, H) * W + x));
    const int dn = grey_u8(rgb + 3 * ((size_t)reflect101(y + 1, H) * W + x));
    const int lf = grey_u8(rgb + 3 * ((size_t)y * W + reflect101(x - 1, W)));
    const int rt = grey_u8(rgb + 3 * ((size_t)y * W + reflect101(x + 1, W)));
    const int lap = up + dn + lf + rt - 4 * c;
    s[0] += lap;
    s[1] += (long long)(lap * lap);
  }
  block_sum0<FR_NT>(s, red);
  if (tid == 0) {
    part[2 * blockIdx.x] = s[0];
    part[2 * blockIdx.x + 1] = s[1];
  }
}

// every workgroup sums the SH_PARTS partials (integers: exact in any order), forms the variance and writes var x mask
// over its share of the loss-weight plane.  var = (N S2 - S1^2) / N^2: the numerator exact in int64, then fp64 (one rounding
// above 2^53), the division in fp64, one rounding to fp32.  numpy's float32 .var() of the same values agrees to ~1e-7.
__global__ __launch_bounds__(FR_NT) void k_frame_weight(const long long* __restrict__ part, int n_px, const unsigned char* __restrict__ motion_mask,
                                                         float* __restrict__ weight) {
  __shared__ long long red[2 * (FR_NT / 64)];
  __shared__ float var_s;
  const int tid = threadIdx.x;
  long long s[2] = {0, 0};
  for (int k = tid; k < SH_PARTS; k += FR_NT) { s[0] += part[2 * k]; s[1] += part[2 * k + 1]; }
  block_sum0<FR_NT>(s, red);
  if (tid == 0) {
    const long long N = n_px;
    const double num = (double)(N * s[1] - s[0] * s[0]);
    var_s = (float)(num / ((double)N * (double)N));
  }
  __syncthreads();
  const float v = var_s;
  for (int i = blockIdx.x * FR_NT + tid; i < n_px; i += gridDim.x * FR_NT)
    weight[i] = motion_mask ? (motion_mask[i] ? v : 0.0f) : v;          // laplacian * mask: a bool mask -> var or 0
}

// the window's own invariants, checked by every entry point before its first launch (nullptr: fine)
static const char* frames_check(const LrfFrameWindow* w) {
  if (!w) return "LrfFrameWindow: null window";
  if (w->capacity <= 0 || w->n_px <= 0 || w->num_images <= 0) return "LrfFrameWindow: capacity, n_px and num_images must be positive";
  if ((long long)w->capacity * w->n_px > (long long)INT32_MAX * 16) return "LrfFrameWindow: window too large";
  if (!w->rgb || !w->loss_weight || !w->slot_of || !w->status) return "LrfFrameWindow: rgb, loss_weight, slot_of and status are required";
  if ((!w->fwd_flow) != (!w->fwd_mask) || (!w->bwd_flow) != (!w->bwd_mask)) return "LrfFrameWindow: a flow plane needs its mask plane";
  return nullptr;
}

}  // namespace lrf

extern "C" int lrf_frames_gather(const LrfFrameWindow* w, const int64_t* view_ids, const int64_t* ray_ids, int32_t V, int32_t n,
                                 float* rgbs, float* loss_weights, float* invdepths, float* fwd_flow, float* fwd_mask,
                                 float* bwd_flow, float* bwd_mask, void* stream) {
  using namespace lrf;
  const char* who = "lrf_frames_gather";
  if (const char* bad = frames_check(w)) return refuse(bad);
  if (V <= 0 || n <= 0 || (long long)V * n > INT32_MAX / 4) return refuse(who, "need V > 0, n > 0 and V * n < 2^29");
  if (!view_ids || !ray_ids) return refuse(who, "null ids");
  if ((invdepths && !w->invdepth) || ((fwd_flow || fwd_mask) && !w->fwd_flow) || ((bwd_flow || bwd_mask) && !w->bwd_flow))
    return refuse(who, "an output was asked for a plane the window does not hold");
  const long long B = (long long)V * n;
  return launch(k_frames_gather, blocks_for(B, FR_NT), FR_NT, reinterpret_cast<hipStream_t>(stream), *w,
                reinterpret_cast<const long long*>(view_ids), reinterpret_cast<const long long*>(ray_ids), V, n,
                rgbs, loss_weights, invdepths, fwd_flow, fwd_mask, bwd_flow, bwd_mask);
}

extern "C" int lrf_decode_flow(const LrfFrameWindow* w, int32_t slot, int32_t backward, const uint16_t* encoded, int32_t H, int32_t W,
                               double flow_scale, void* stream) {
  using namespace lrf;
  const char* who = "lrf_decode_flow";
  if (const char* bad = frames_check(w)) return refuse(bad);
  if (slot < 0 || slot >= w->capacity) return refuse(who, "slot outside the window");
  if (H <= 0 || W <= 0 || (long long)H * W != w->n_px) return refuse(who, "H * W must equal the window's n_px");
  if (!encoded) return refuse(who, "null encoded flow");
  float* flow = backward ? w->bwd_flow : w->fwd_flow;
  float* mask = backward ? w->bwd_mask : w->fwd_mask;
  if (!flow) return refuse(who, "the window holds no flow planes");
  const float scale = (float)flow_scale;                      // numpy: float32 array * Python float -> the float rounded to fp32
  if (!__builtin_isfinite(scale)) return refuse(who, "flow_scale must be finite in fp32");
  const size_t off = (size_t)slot * w->n_px;
  return launch(k_decode_flow, blocks_for(w->n_px, FR_NT), FR_NT, reinterpret_cast<hipStream_t>(stream),
                reinterpret_cast<const unsigned short*>(encoded), w->n_px, scale, flow + 2 * off, mask + off);
}

// [SH_PARTS x (sum, sum of squares)]; its size is c.at, not rounded
static long long* carve_sharpness(lrf::Carver& c) { return c.take<long long>((size_t)lrf::SH_PARTS * 2); }

extern "C" size_t lrf_frame_sharpness_workspace_bytes(void) {
  lrf::Carver c(nullptr);
  carve_sharpness(c);
  return c.at;
}

extern "C" int lrf_frame_sharpness(const LrfFrameWindow* w, int32_t slot, int32_t H, int32_t W, const uint8_t* motion_mask,
                                   void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_frame_sharpness";
  if (const char* bad = frames_check(w)) return refuse(bad);
  if (slot < 0 || slot >= w->capacity) return refuse(who, "slot outside the window");
  if (H <= 0 || W <= 0 || (long long)H * W != w->n_px) return refuse(who, "H * W must equal the window's n_px");
  if (w->n_px > SH_MAX_PX) return refuse(who, "at most 2^21 pixels per frame (the int64 variance bound)");
  if (!workspace) return refuse(who, "null workspace");
  const size_t off = (size_t)slot * w->n_px;
  Carver c(workspace);
  long long* part = carve_sharpness(c);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_frame_sharpness, SH_PARTS, FR_NT, st, w->rgb + 3 * off, H, W, part));
  const unsigned blocks = blocks_for(w->n_px, FR_NT * 8);
  return launch(k_frame_weight, blocks < 1024 ? blocks : 1024, FR_NT, st, part, w->n_px,
                reinterpret_cast<const unsigned char*>(motion_mask), w->loss_weight + off);
}
