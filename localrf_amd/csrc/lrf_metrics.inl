// lrf_metrics.inl -- test-view image metrics (included by lrf_render.hip): per-frame MSE and the mip-NeRF SSIM of
// utils/utils.py:232-287 (rgb_ssim), for a batch of B frame pairs [B,H,W,3] (contiguous fp32, HWC).
//
// SSIM follows the reference's arithmetic: the filter taps and the even-size shift are built on the host in fp64
// (lrf_image_metrics); each moment image x, y, x^2, y^2, xy (the squares and the product rounded in fp32, as numpy forms
// them from the renderer's fp32 arrays, then widened) is blurred in fp64 along the rows' axis first (filt[:, None]), then
// along the columns (filt[None, :]), both as scipy.signal.convolve2d(mode="valid") -- a true convolution, so tap k of
// the filter weights input offset fs-1-k.  fp64 throughout: in fp32, E[x^2] - mu^2 cancels to errors near 1e-4 of the map.
//
// k_img_metrics: one workgroup of MT_NT threads per MT_TW x MT_TH tile of OWNED pixels of one frame; the grid covers
// the whole image.  Per channel it stages both images' (MT_TH+fs-1) x (MT_TW+fs-1) fp32 window in LDS, then, in strips of
// MT_RS rows, runs the vertical pass into an fp64 LDS buffer (5 moments) and the horizontal pass, SSIM and the sums in
// registers.  A pixel's squared error counts once, in the tile that owns it; its SSIM counts when it is also a valid
// output position (y < H-fs+1, x < W-fs+1).  Each workgroup writes one (ssim sum, squared-error sum) partial;
// k_img_metrics_reduce sums a frame's partials in tile order.  No atomics: the results are bit-identical from run to
// run and do not depend on B.  LDS at fs = 31: 2 x 46 x 94 x 4 + 5 x 8 x 94 x 8 = 64,672 bytes (below the 64 KiB that
// needs no opt-in); at fs = 11, 39 KB.
namespace lrf {

constexpr int MT_TW = 64;        // owned columns per tile (one wave64 row in the horizontal pass: consecutive doubles, no bank conflict)
constexpr int MT_TH = 16;        // owned rows per tile
constexpr int MT_RS = 8;         // rows per strip of the fp64 vertical-pass buffer
constexpr int MT_NT = 256;
constexpr int MT_MAX_FS = 31;

struct MetricsArgs {
  const float* img0; const float* img1;
  double* map;                   // [B, OH, OW, 3] or null
  double2* part;                 // [B, tiles]: (ssim sum, squared-error sum)
  int H, W, fs, OH, OW, tiles_x, tiles;
  double c1, c2;
  double taps[MT_MAX_FS + 1];    // taps[k] = filt[fs-1-k]: weight of input offset k (convolution)
};

__device__ inline double nan_min(double a, double b) { return (a != a || b != b) ? a + b : (a < b ? a : b); }   // np.minimum
__device__ inline double np_sign(double a) { return a > 0.0 ? 1.0 : (a < 0.0 ? -1.0 : a); }                       // sign(0) = 0, sign(NaN) = NaN

__global__ __launch_bounds__(MT_NT) void k_img_metrics(MetricsArgs a) {
  extern __shared__ double mt_lds[];
  const int fs = a.fs, EW = MT_TW + fs - 1, EH = MT_TH + fs - 1;
  double* sm = mt_lds;                                               // [5][MT_RS][EW] vertical-pass moments
  float* sx = reinterpret_cast<float*>(mt_lds + 5 * MT_RS * EW);     // [EH][EW] window of img0, one channel
  float* sy = sx + EH * EW;                                          // ... of img1
  __shared__ double taps[MT_MAX_FS + 1];
  __shared__ double red[2 * (MT_NT / 64)];

  const int tid = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int y0 = ty * MT_TH, x0 = tx * MT_TW;
  const size_t frame = (size_t)b * a.H * a.W * 3;
  const float* p0 = a.img0 + frame;
  const float* p1 = a.img1 + frame;
  if (tid < fs) taps[tid] = a.taps[tid];

  double ssim_acc = 0.0, sq_acc = 0.0;
  for (int c = 0; c < 3; ++c) {
    __syncthreads();                                                 // previous channel's readers are done with sx / sy / sm
    for (int i = tid; i < EH * EW; i += MT_NT) {
      const int r = i / EW, q = i - r * EW;
      const int gy = y0 + r, gx = x0 + q;
      float u = 0.0f, v = 0.0f;                                      // outside the image: feeds invalid outputs only
      if (gy < a.H && gx < a.W) {
        const size_t o = ((size_t)gy * a.W + gx) * 3 + c;
        u = p0[o]; v = p1[o];
      }
      sx[i] = u; sy[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < MT_TH * MT_TW; i += MT_NT) {               // squared error of the owned pixels, fixed order per thread
      const int r = i / MT_TW, q = i - r * MT_TW;
      if (y0 + r < a.H && x0 + q < a.W) {
        const double d = (double)sx[r * EW + q] - (double)sy[r * EW + q];
        sq_acc += d * d;
      }
    }
    for (int r0 = 0; r0 < MT_TH; r0 += MT_RS) {
      if (r0 > 0) __syncthreads();                                   // the previous strip's horizontal pass has read sm
      for (int i = tid; i < MT_RS * EW; i += MT_NT) {                // vertical pass (convolve2d with filt[:, None])
        const int r = i / EW, q = i - r * EW;
        const float* wx = sx + (r0 + r) * EW + q;
        const float* wy = sy + (r0 + r) * EW + q;
        double m0 = 0.0, m1 = 0.0, m00 = 0.0, m11 = 0.0, m01 = 0.0;
        for (int k = 0; k < fs; ++k) {
          const float u = wx[k * EW], v = wy[k * EW];
          const double t = taps[k];
          m0 += t * (double)u;
          m1 += t * (double)v;
          m00 += t * (double)(u * u);                                // img0**2 of an fp32 array is fp32
          m11 += t * (double)(v * v);
          m01 += t * (double)(u * v);
        }
        const int o = r * EW + q;
        sm[o] = m0; sm[MT_RS * EW + o] = m1; sm[2 * MT_RS * EW + o] = m00;
        sm[3 * MT_RS * EW + o] = m11; sm[4 * MT_RS * EW + o] = m01;
      }
      __syncthreads();
      for (int i = tid; i < MT_RS * MT_TW; i += MT_NT) {             // horizontal pass (filt[None, :]) and SSIM
        const int r = i / MT_TW, q = i - r * MT_TW;
        const int oy = y0 + r0 + r, ox = x0 + q;
        if (oy >= a.OH || ox >= a.OW) continue;
        const double* w = sm + r * EW + q;
        double mu0 = 0.0, mu1 = 0.0, e00 = 0.0, e11 = 0.0, e01 = 0.0;
        for (int k = 0; k < fs; ++k) {
          const double t = taps[k];
          mu0 += t * w[k];
          mu1 += t * w[MT_RS * EW + k];
          e00 += t * w[2 * MT_RS * EW + k];
          e11 += t * w[3 * MT_RS * EW + k];
          e01 += t * w[4 * MT_RS * EW + k];
        }
        // utils.py:266-285
        const double mu00 = mu0 * mu0, mu11 = mu1 * mu1, mu01 = mu0 * mu1;
        double s00 = e00 - mu00, s11 = e11 - mu11, s01 = e01 - mu01;
        s00 = s00 < 0.0 ? 0.0 : s00;                                 // np.maximum(0, s): NaN stays NaN
        s11 = s11 < 0.0 ? 0.0 : s11;
        s01 = np_sign(s01) * nan_min(sqrt(s00 * s11), fabs(s01));
        const double numer = (2.0 * mu01 + a.c1) * (2.0 * s01 + a.c2);
        const double denom = (mu00 + mu11 + a.c1) * (s00 + s11 + a.c2);
        const double v = numer / denom;
        if (a.map) a.map[(((size_t)b * a.OH + oy) * a.OW + ox) * 3 + c] = v;
        ssim_acc += v;
      }
    }
  }
  double acc[2] = {ssim_acc, sq_acc};
  block_sum0<MT_NT>(acc, red);                                        // the fixed order of lrf_common.h
  if (tid == 0) a.part[(size_t)b * a.tiles + tile] = make_double2(acc[0], acc[1]);
}

// one workgroup per frame: thread t sums tiles t, t + MT_NT, ... in order, then the same fixed-order reduction
__global__ __launch_bounds__(MT_NT) void k_img_metrics_reduce(const double2* __restrict__ part, int tiles, double n_ssim, double n_px,
                                                              double* __restrict__ ssim_mean, double* __restrict__ mse) {
  __shared__ double red[2 * (MT_NT / 64)];
  const int tid = threadIdx.x, b = blockIdx.x;
  double acc[2] = {0.0, 0.0};
  for (int t = tid; t < tiles; t += MT_NT) {
    const double2 p = part[(size_t)b * tiles + t];
    acc[0] += p.x; acc[1] += p.y;
  }
  block_sum0<MT_NT>(acc, red);
  if (tid == 0) {
    ssim_mean[b] = acc[0] / n_ssim;
    mse[b] = acc[1] / n_px;
  }
}

static void metrics_tiles(int H, int W, int* tiles_x, int* tiles) {
  *tiles_x = (W + MT_TW - 1) / MT_TW;
  *tiles = *tiles_x * ((H + MT_TH - 1) / MT_TH);
}
// [B x tiles partial sums]; its size is c.at, not rounded
static double2* carve_metrics(Carver& c, int B, int tiles) { return c.take<double2>((size_t)B * tiles); }

}  // namespace lrf

extern "C" size_t lrf_image_metrics_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t filter_size) {
  using namespace lrf;
  if (B <= 0 || H <= 0 || W <= 0 || filter_size < 1 || filter_size > MT_MAX_FS || H < filter_size || W < filter_size ||
      (long long)H * W * 3 > INT32_MAX / 2) return 0;
  int tx, tiles;
  metrics_tiles(H, W, &tx, &tiles);
  Carver c(nullptr);
  carve_metrics(c, B, tiles);
  return c.at;
}

extern "C" int lrf_image_metrics(const LrfImageMetrics* m, double* ssim_map, double* ssim_mean, double* mse, void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_image_metrics";
  if (!m) return refuse(who, "null argument");
  const int B = m->B, H = m->H, W = m->W, fs = m->filter_size;
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0) return refuse(who, "need 1 <= B <= 65535, H > 0 and W > 0");
  if ((long long)H * W * 3 > INT32_MAX / 2) return refuse(who, "frame too large (H * W * 3 must stay below 2^30)");
  if (fs < 1 || fs > MT_MAX_FS) return refuse(who, "filter_size must lie in 1..31");
  if (H < fs || W < fs) return refuse(who, "H and W must be at least filter_size (the valid SSIM map would be empty)");
  if (m->filter_sigma == 0.0 || !__builtin_isfinite(m->filter_sigma)) return refuse(who, "filter_sigma must be finite and non-zero");
  if (!__builtin_isfinite(m->max_val) || !__builtin_isfinite(m->k1) || !__builtin_isfinite(m->k2))
    return refuse(who, "max_val, k1 and k2 must be finite");
  if (!m->img0 || !m->img1 || !ssim_mean || !mse || !workspace) return refuse(who, "null argument");

  MetricsArgs a;
  memset(&a, 0, sizeof(a));
  // utils.py:246-251, in fp64; np.sum's pairwise order for the normalisation (8 accumulators from 8 entries on)
  const int hw = fs / 2;
  const double shift = (2 * hw - fs + 1) / 2.0;
  double filt[MT_MAX_FS + 1];
  for (int i = 0; i < fs; ++i) {
    const double x = ((double)(i - hw) + shift) / m->filter_sigma;
    filt[i] = exp(-0.5 * (x * x));
  }
  double sum = 0.0;
  if (fs < 8) {
    for (int i = 0; i < fs; ++i) sum += filt[i];
  } else {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = filt[j];
    int i = 8;
    for (; i + 8 <= fs; i += 8)
      for (int j = 0; j < 8; ++j) r[j] += filt[i + j];
    sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < fs; ++i) sum += filt[i];
  }
  if (!(sum > 0.0) || !__builtin_isfinite(sum)) return refuse(who, "the Gaussian filter vanishes (filter_sigma too small)");
  for (int k = 0; k < fs; ++k) a.taps[k] = filt[fs - 1 - k] / sum;

  a.img0 = m->img0; a.img1 = m->img1; a.map = ssim_map;
  a.H = H; a.W = W; a.fs = fs; a.OH = H - fs + 1; a.OW = W - fs + 1;
  metrics_tiles(H, W, &a.tiles_x, &a.tiles);
  Carver c(workspace);
  a.part = carve_metrics(c, B, a.tiles);
  const double c1 = m->k1 * m->max_val, c2 = m->k2 * m->max_val;
  a.c1 = c1 * c1; a.c2 = c2 * c2;
  const int EW = MT_TW + fs - 1, EH = MT_TH + fs - 1;
  const size_t lds = (size_t)5 * MT_RS * EW * sizeof(double) + (size_t)2 * EH * EW * sizeof(float);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch_lds(k_img_metrics, dim3(a.tiles, B), MT_NT, lds, st, a));
  return launch(k_img_metrics_reduce, B, MT_NT, st, a.part, a.tiles, (double)a.OH * a.OW * 3, (double)H * W * 3, ssim_mean, mse);
}
