// lrf_evalgeo.inl -- the geometry diagnostics renderer.render(test=True) builds per test view (renderer.py:79-124), for a
// batch of V views (included by lrf_render.hip after lrf_losses.inl and lrf_select.inl):
//
//   lrf_flow_comparison   predicted forward / backward flow of every pixel (utils.py:15-48 through make_cam2cam /
//                         reproject of lrf_losses.inl), laid out as renderer.py:91-114 stacks it: image [3H, 2W], column
//                         half c = flow component c, rows 0..H the prediction, H..2H the dataset flow, 2H..3H
//                         |pred - flow| * mask / W.  Rows 0..2H of each half are divided by np.quantile(those rows, 0.9)
//                         (lrf_select, bit for bit); then the whole image is clamped to [0, 1] (NaN stays NaN).
//   lrf_depth_comparison  compute_depth_loss (utils.py:50-59) over the whole frame: x = 1 / clamp(depth, 1e-6), y = the
//                         dataset inverse depth; t = torch.median (lrf_select), s = mean |. - t| summed in fp64 in a fixed
//                         order and rounded once to fp32 (torch: an fp32 mean); image [3H, W] = vstack(0.5 x^, 0.5 y^,
//                         (x^ - y^)^2) clamped to [0, 1].
//
// The launch count does not depend on V: flow 2 + one select (11), depth 4 + one select (10).  Elementwise arithmetic is
// fp32 with the reference's operation order; the kernels that form the images turn contraction off.  The
// reprojection is lrf_losses.inl's (contracted), within ~1 ulp of the reference's bmm.
namespace lrf {

constexpr int EG_NT = 256;
constexpr float EG_FLOW_Q = 0.9f;        // renderer.py:93 np.quantile(., 0.9), q rounded to fp32 as numpy does

struct FlowCmpArgs {
  const float* c2w; const float* depth; const float* dirs; const long long* ij;
  const float* flow[2]; const float* mask[2];
  const float* focal; const float* center;
  float* raw[2];                         // [V, 3H, 2W]
  float* sel;                            // [V, 4, 2HW]: the select rows (fwd c0, fwd c1, bwd c0, bwd c1)
  int F, V, H, W;
  int idx[LRF_EVAL_MAX_VIEWS];
};

__device__ __forceinline__ float clamp01_nan(float v) { return v != v ? v : fminf(fmaxf(v, 0.0f), 1.0f); }

__global__ __launch_bounds__(EG_NT) void k_flow_cmp(FlowCmpArgs a) {
#pragma clang fp contract(off)
  __shared__ Cam2Cam cc[2];
  const int v = blockIdx.y, HW = a.H * a.W;
  const int idx = a.idx[v];
  if (threadIdx.x < 2) {                                           // utils.py:29-41: neighbours clamp(idx +- 1, 0, F - 1)
    const int nb = threadIdx.x == 0 ? min(idx + 1, a.F - 1) : max(idx - 1, 0);
    cc[threadIdx.x] = make_cam2cam(a.c2w + (size_t)nb * 12, a.c2w + (size_t)idx * 12);
  }
  __syncthreads();
  const int p = blockIdx.x * EG_NT + threadIdx.x;
  if (p >= HW) return;
  const size_t vp = (size_t)v * HW + p;
  const float d = a.depth[vp];
  const float pt[3] = {a.dirs[vp * 3] * d, a.dirs[vp * 3 + 1] * d, a.dirs[vp * 3 + 2] * d};
  const float col = (float)a.ij[vp * 2], row = (float)a.ij[vp * 2 + 1];
  const float f = a.focal[0], cx = a.center[0], cy = a.center[1];
  const int y = p / a.W, x = p - y * a.W;
  const float Wf = (float)a.W;
  for (int dir = 0; dir < 2; ++dir) {
    const Reproj r = reproject(cc[dir], pt, f, cx, cy, col, row);
    const float m = a.mask[dir][vp];
    float* img = a.raw[dir] + (size_t)v * 6 * HW;
    for (int c = 0; c < 2; ++c) {
      const float pred = c == 0 ? r.fx : r.fy;
      const float fl = a.flow[dir][vp * 2 + c];
      const float err = fabsf(pred - fl) * m / Wf;
      const size_t o = (size_t)y * 2 * a.W + (size_t)c * a.W + x;
      img[o] = pred;
      img[o + (size_t)2 * HW] = fl;                                // row H + y
      img[o + (size_t)4 * HW] = err;                               // row 2H + y
      float* s = a.sel + ((size_t)v * 4 + dir * 2 + c) * 2 * HW;
      s[p] = pred;
      s[HW + p] = fl;
    }
  }
}

// out = clamp(raw / q) on rows 0..2H, clamp(raw) below; q = quant[v, dir, column half].  out may alias raw.
__global__ __launch_bounds__(EG_NT) void k_flow_norm(const float* raw0, const float* raw1, float* out0, float* out1,
                                                     const float* __restrict__ quant, int H, int W) {
#pragma clang fp contract(off)
  const int v = blockIdx.y >> 1, dir = blockIdx.y & 1;
  const int e = blockIdx.x * EG_NT + threadIdx.x;
  const int n = 6 * H * W;
  if (e >= n) return;
  const int row = e / (2 * W), col = e - row * 2 * W;
  const size_t o = (size_t)v * n + e;
  float val = (dir ? raw1 : raw0)[o];
  if (row < 2 * H) val = val / quant[v * 4 + dir * 2 + (col >= W)];
  (dir ? out1 : out0)[o] = clamp01_nan(val);
}

// rows 0..V of sel: x = 1 / clamp(depth, 1e-6); rows V..2V: y (the dataset inverse depth)
__global__ __launch_bounds__(EG_NT) void k_depth_prep(const float* __restrict__ depth, const float* __restrict__ inv, float* __restrict__ sel,
                                                      int V, int HW) {
#pragma clang fp contract(off)
  const int v = blockIdx.y, p = blockIdx.x * EG_NT + threadIdx.x;
  if (p >= HW) return;
  const size_t vp = (size_t)v * HW + p;
  const float d = depth[vp];
  sel[vp] = 1.0f / (d != d ? d : fmaxf(d, 1e-6f));
  sel[(size_t)V * HW + vp] = inv[vp];
}

// per (row, chunk of EG_NT * 16 values): fp64 sum of the fp32 |x - t|, fixed order (thread-strided, then block_sum0)
__global__ __launch_bounds__(EG_NT) void k_depth_mad(const float* __restrict__ sel, const float* __restrict__ med, double* __restrict__ part,
                                                     int HW, int chunks) {
  __shared__ double red[EG_NT / 64];
  const int r = blockIdx.y, tid = threadIdx.x;
  const float t = med[r];
  const float* p = sel + (size_t)r * HW;
  double s = 0.0;
  for (int k = 0; k < 16; ++k) {
    const int i = (blockIdx.x * 16 + k) * EG_NT + tid;
    if (i < HW) s += (double)fabsf(__fsub_rn(p[i], t));
  }
  const double q = block_sum0<EG_NT>(s, red);
  if (tid == 0) part[(size_t)r * chunks + blockIdx.x] = q;
}

// one workgroup per row: the row's partials in order; stats[v] = (t_x, t_y, s_x, s_y)
__global__ __launch_bounds__(EG_NT) void k_depth_mad_reduce(const double* __restrict__ part, const float* __restrict__ med, int chunks,
                                                            int V, double n, float* __restrict__ stats) {
  __shared__ double red[EG_NT / 64];
  const int r = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int c = tid; c < chunks; c += EG_NT) s += part[(size_t)r * chunks + c];
  const double q = block_sum0<EG_NT>(s, red);
  if (tid == 0) {
    const int v = r % V, which = r / V;                            // 0: x (rendered), 1: y (dataset)
    stats[v * 4 + which] = med[r];
    stats[v * 4 + 2 + which] = (float)(q / n);
  }
}

__global__ __launch_bounds__(EG_NT) void k_depth_out(const float* __restrict__ sel, const float* __restrict__ stats, float* __restrict__ out,
                                                     int V, int HW) {
#pragma clang fp contract(off)
  const int v = blockIdx.y, p = blockIdx.x * EG_NT + threadIdx.x;
  if (p >= HW) return;
  const size_t vp = (size_t)v * HW + p;
  const float* st = stats + v * 4;
  const float xn = (sel[vp] - st[0]) / st[2];
  const float yn = (sel[(size_t)V * HW + vp] - st[1]) / st[3];
  const float d = xn - yn;
  float* o = out + (size_t)v * 3 * HW;
  o[p] = clamp01_nan(0.5f * xn);
  o[HW + p] = clamp01_nan(0.5f * yn);
  o[2 * HW + p] = clamp01_nan(d * d);
}

static bool eg_frame_ok(int H, int W) { return H > 0 && W > 0 && (long long)H * W * 6 < (1ll << 31); }
static int depth_chunks(int HW) { return (HW + EG_NT * 16 - 1) / (EG_NT * 16); }

// [select of 4 V rows] [the 8 V H W floats it selects from]
struct FlowCmpWs { void* select; float* sel; size_t bytes; };
static FlowCmpWs carve_flow_cmp(void* ws, int V, int HW) {
  FlowCmpWs w;
  Carver c(ws);
  w.select = c.take<char>(select_ws_bytes(4 * V));
  w.sel = c.take<float>((size_t)V * 8 * HW, 256);
  w.bytes = c.bytes();
  return w;
}
// [select of 2 V rows] [2 V H W floats] [2 V chunks partial sums] [2 V medians]
struct DepthCmpWs { void* select; float* sel; double* part; float* med; size_t bytes; };
static DepthCmpWs carve_depth_cmp(void* ws, int V, int HW) {
  DepthCmpWs w;
  Carver c(ws);
  w.select = c.take<char>(select_ws_bytes(2 * V));
  w.sel = c.take<float>((size_t)2 * V * HW, 256);
  w.part = c.take<double>((size_t)2 * V * depth_chunks(HW), 256);
  w.med = c.take<float>((size_t)2 * V, 256);
  w.bytes = c.bytes();
  return w;
}

}  // namespace lrf

extern "C" size_t lrf_flow_comparison_workspace_bytes(int32_t V, int32_t H, int32_t W) {
  using namespace lrf;
  if (V < 1 || V > LRF_EVAL_MAX_VIEWS || !eg_frame_ok(H, W)) return 0;
  return carve_flow_cmp(nullptr, V, H * W).bytes;
}

extern "C" int lrf_flow_comparison(const LrfFlowComparison* c, float* fwd_cmp, float* bwd_cmp, float* fwd_raw, float* bwd_raw,
                                   float* quantiles, void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_flow_comparison";
  if (!c) return refuse(who, "null argument");
  const int V = c->V, H = c->H, W = c->W, F = c->F;
  if (V < 1 || V > LRF_EVAL_MAX_VIEWS) return refuse(who, "need 1 <= V <= LRF_EVAL_MAX_VIEWS");
  if (!eg_frame_ok(H, W)) return refuse(who, "need H, W > 0 and 6 H W < 2^31");
  if (F < 1) return refuse(who, "need F >= 1 poses");
  for (int v = 0; v < V; ++v)
    if (c->idx[v] < 0 || c->idx[v] >= F) return refuse(who, "a view index lies outside [0, F)");
  if (!c->cam2world || !c->depth || !c->dirs || !c->ij || !c->fwd_flow || !c->fwd_mask || !c->bwd_flow || !c->bwd_mask ||
      !c->focal || !c->center || !fwd_cmp || !bwd_cmp || !quantiles || !workspace)
    return refuse(who, "null argument");
  if ((fwd_raw == nullptr) != (bwd_raw == nullptr)) return refuse(who, "fwd_raw and bwd_raw go together");

  const int HW = H * W;
  const FlowCmpWs w = carve_flow_cmp(workspace, V, HW);
  FlowCmpArgs a;
  memset(&a, 0, sizeof(a));
  a.c2w = c->cam2world; a.depth = c->depth; a.dirs = c->dirs; a.ij = reinterpret_cast<const long long*>(c->ij);
  a.flow[0] = c->fwd_flow; a.flow[1] = c->bwd_flow; a.mask[0] = c->fwd_mask; a.mask[1] = c->bwd_mask;
  a.focal = c->focal; a.center = c->center;
  a.raw[0] = fwd_raw ? fwd_raw : fwd_cmp; a.raw[1] = bwd_raw ? bwd_raw : bwd_cmp;
  a.sel = w.sel;
  a.F = F; a.V = V; a.H = H; a.W = W;
  for (int v = 0; v < V; ++v) a.idx[v] = c->idx[v];
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_flow_cmp, dim3(blocks_for(HW, EG_NT), V), EG_NT, st, a));
  const int64_t n = 2ll * HW;
  LRF_TRY(select_launch(a.sel, n, &n, 1, 4 * V, LRF_SELECT_QUANTILE, EG_FLOW_Q, quantiles, w.select, st));
  return launch(k_flow_norm, dim3(blocks_for(6ll * HW, EG_NT), 2 * V), EG_NT, st, a.raw[0], a.raw[1], fwd_cmp, bwd_cmp, quantiles, H, W);
}

extern "C" size_t lrf_depth_comparison_workspace_bytes(int32_t V, int32_t H, int32_t W) {
  using namespace lrf;
  if (V < 1 || V > 32767 || !eg_frame_ok(H, W)) return 0;
  return carve_depth_cmp(nullptr, V, H * W).bytes;
}

extern "C" int lrf_depth_comparison(const float* depth, const float* invdepth, int32_t V, int32_t H, int32_t W, float* out, float* stats,
                                    void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_depth_comparison";
  if (V < 1 || V > 32767) return refuse(who, "need 1 <= V <= 32767");
  if (!eg_frame_ok(H, W)) return refuse(who, "need H, W > 0 and 6 H W < 2^31");
  if (!depth || !invdepth || !out || !stats || !workspace) return refuse(who, "null argument");
  const int HW = H * W, chunks = depth_chunks(HW);
  const DepthCmpWs w = carve_depth_cmp(workspace, V, HW);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_depth_prep, dim3(blocks_for(HW, EG_NT), V), EG_NT, st, depth, invdepth, w.sel, V, HW));
  const int64_t n = HW;
  LRF_TRY(select_launch(w.sel, n, &n, 1, 2 * V, LRF_SELECT_MEDIAN, 0.0f, w.med, w.select, st));
  LRF_TRY(launch(k_depth_mad, dim3(chunks, 2 * V), EG_NT, st, w.sel, w.med, w.part, HW, chunks));
  LRF_TRY(launch(k_depth_mad_reduce, 2 * V, EG_NT, st, w.part, w.med, chunks, V, (double)HW, stats));
  return launch(k_depth_out, dim3(blocks_for(HW, EG_NT), V), EG_NT, st, w.sel, stats, out, V, HW);
}
