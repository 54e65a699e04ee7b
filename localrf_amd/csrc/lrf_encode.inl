// lrf_encode.inl -- byte encoding of rendered frames (included by lrf_render.hip): what renderer.render(test=False) writes
// per frame (renderer.py:130-148,172-174), for V frames of H x W pixels in one launch (two with the automatic depth range).
//
//   rgb8       cv2.imwrite(255 * rgb): saturate_cast<uchar>(fp32(255 * x)) = clamp(rint(255 * x), 0, 255), ties to even;
//              NaN -> 0.  The channels keep the input's (RGB) order.
//   depth_idx  the index image visualize_depth (utils/utils.py:179-197) hands to cv2.applyColorMap, in numpy 2.2's fp32
//              arithmetic: x = nan_to_num(d) (NaN -> 0, +-inf -> +-FLT_MAX); t = fp32(x - mi) / D (IEEE division);
//              idx = uint8(fp32(255 * clip(t, 0, 1))), truncated; a NaN t (an inf / inf, or mi = NaN when the automatic range
//              found no positive depth) gives 0, as numpy's cast does on x86.
//   depth8     lut[depth_idx], three bytes per pixel in the table's own channel order.
//
// The automatic range (visualize_depth(minmax=None)): mi = min(x[x > 0]), ma = max(x), D = fp32(fp32(ma - mi) + 1e-8f).
// k_encode_range writes each frame's per-workgroup extrema as order-preserving uint32 keys to the workspace (integer
// min / max only, every slot written, no atomics across workgroups); k_encode reduces the partials of the frames its pixels
// belong to in LDS, so the result does not depend on scheduling.  A fixed range arrives as (mi, D) already rounded to fp32
// by the caller, as numpy rounds a Python number.
//
// k_encode: one lane per 4 pixels (three float4 rgb loads, one float4 depth load; 12 + 12 + 4 bytes out as dword stores),
// the LUT packed as 256 uint32 in LDS (one ds_read_b32 per pixel), a scalar tail for V H W % 4.  Contraction is off.
namespace lrf {

constexpr int ENC_NT = 256;
constexpr int ENC_PX = 4 * ENC_NT;                       // pixels per k_encode workgroup
constexpr int ENC_RANGE_WG = 64;                         // k_encode_range workgroups per frame (one partial each)
constexpr int ENC_MAX_FRAMES_WG = ENC_PX + 1;            // frames one k_encode workgroup can touch (H W = 1)
constexpr unsigned ENC_NO_POS = 0xFFFFFFFFu;             // min key of a frame without a positive depth

// nan_to_num, then -0.0 -> +0.0; the bits of the result
__device__ __forceinline__ unsigned enc_clean_bits(float d) {
  unsigned u = __float_as_uint(d);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;                           // NaN -> 0
  if ((u & 0x7FFFFFFFu) == 0x7F800000u) return (u & 0x80000000u) | 0x7F7FFFFFu;   // +-inf -> +-FLT_MAX
  return u == 0x80000000u ? 0u : u;
}
__device__ __forceinline__ unsigned enc_key(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ unsigned enc_unkey(unsigned k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

// ws[(v * ENC_RANGE_WG + b) * 2] = {min key over the positive values, max key over all values} of workgroup b's share
__global__ __launch_bounds__(ENC_NT) void k_encode_range(const float* __restrict__ depth, int HW, unsigned* __restrict__ ws) {
  __shared__ unsigned red[2][ENC_NT / 64];
  const int v = blockIdx.y, b = blockIdx.x;
  const float* d = depth + (size_t)v * HW;
  unsigned mn = ENC_NO_POS, mx = 0u;
  for (int p = b * ENC_NT + threadIdx.x; p < HW; p += ENC_RANGE_WG * ENC_NT) {
    const unsigned u = enc_clean_bits(d[p]);
    if (u != 0u && !(u & 0x80000000u)) mn = min(mn, u);                    // x > 0: a positive float's bits keep its order
    mx = max(mx, enc_key(u));
  }
  mn = block_min0<ENC_NT>(mn, red[0]);
  mx = block_max0<ENC_NT>(mx, red[1]);
  if (threadIdx.x == 0) {
    ws[((size_t)v * ENC_RANGE_WG + b) * 2] = mn;
    ws[((size_t)v * ENC_RANGE_WG + b) * 2 + 1] = mx;
  }
}

struct EncodeArgs {
  const float* rgb; const float* depth; const uint8_t* lut;
  uint8_t* rgb8; uint8_t* depth8; uint8_t* idx;         // rgb / rgb8 and idx nullable
  float* range_out;                                      // [V, 2] nullable
  const unsigned* ws;                                    // auto range: the k_encode_range partials
  int n;                                                 // V H W (3 V H W < 2^31)
  int HW, V;
  float mi, ma, D;                                       // fixed range
};

__device__ __forceinline__ unsigned enc_rgb_byte(float x) {
#pragma clang fp contract(off)
  const float v = rintf(255.0f * x);                     // ties to even
  return (unsigned)fminf(fmaxf(v, 0.0f), 255.0f);        // fmaxf(NaN, 0) = 0
}

__device__ __forceinline__ unsigned enc_depth_idx(float d, float mi, float D) {
#pragma clang fp contract(off)
  const float x = __uint_as_float(enc_clean_bits(d));
  const float t = (x - mi) / D;                          // IEEE division (no reciprocal)
  return (unsigned)(255.0f * fminf(fmaxf(t, 0.0f), 1.0f));   // a NaN t clamps to 0
}

template <bool AUTO>
__global__ __launch_bounds__(ENC_NT) void k_encode(EncodeArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned lut[256];
  __shared__ float2 rng[AUTO ? ENC_MAX_FRAMES_WG : 1];  // (mi, D) of the frames this workgroup touches
  const int p_begin = blockIdx.x * ENC_PX;
  const int p_end = min(a.n, p_begin + ENC_PX);
  const int f0 = p_begin / a.HW;
  {
    const int t = threadIdx.x;                           // ENC_NT == 256 entries
    lut[t] = (unsigned)a.lut[3 * t] | ((unsigned)a.lut[3 * t + 1] << 8) | ((unsigned)a.lut[3 * t + 2] << 16);
  }
  if (AUTO) {
    const int f1 = (p_end - 1) / a.HW;
    const int lane = threadIdx.x & 63;
    for (int f = f0 + (threadIdx.x >> 6); f <= f1; f += ENC_NT / 64) {   // one wave per frame, one partial per lane
      unsigned mn = a.ws[((size_t)f * ENC_RANGE_WG + lane) * 2], mx = a.ws[((size_t)f * ENC_RANGE_WG + lane) * 2 + 1];
      mn = wave_min(mn);
      mx = wave_max(mx);
      if (lane == 0) {
        const float mi = mn == ENC_NO_POS ? __uint_as_float(0x7FC00000u) : __uint_as_float(mn);
        const float ma = __uint_as_float(enc_unkey(mx));
        const float D = (ma - mi) + 1e-8f;               // numpy: fp32(ma - mi), then + 1e-8 rounded to fp32
        rng[f - f0] = make_float2(mi, D);
        if (a.range_out && f * a.HW >= p_begin) {   // the workgroup holding the frame's first pixel
          a.range_out[2 * f] = mi;
          a.range_out[2 * f + 1] = ma;
        }
      }
    }
  } else if (blockIdx.x == 0 && a.range_out) {
    for (int f = threadIdx.x; f < a.V; f += ENC_NT) {
      a.range_out[2 * f] = a.mi;
      a.range_out[2 * f + 1] = a.ma;
    }
  }
  __syncthreads();

  const int p = p_begin + 4 * threadIdx.x;
  if (p >= p_end) return;
  if (p + 4 <= a.n) {
    if (a.rgb) {
      const float4* r4 = reinterpret_cast<const float4*>(a.rgb + 3 * p);
      const float4 c0 = r4[0], c1 = r4[1], c2 = r4[2];
      const unsigned b[12] = {enc_rgb_byte(c0.x), enc_rgb_byte(c0.y), enc_rgb_byte(c0.z), enc_rgb_byte(c0.w),
                              enc_rgb_byte(c1.x), enc_rgb_byte(c1.y), enc_rgb_byte(c1.z), enc_rgb_byte(c1.w),
                              enc_rgb_byte(c2.x), enc_rgb_byte(c2.y), enc_rgb_byte(c2.z), enc_rgb_byte(c2.w)};
      unsigned* o = reinterpret_cast<unsigned*>(a.rgb8 + 3 * p);
      o[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      o[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
      o[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    }
    const float4 dd = *reinterpret_cast<const float4*>(a.depth + p);
    const float d[4] = {dd.x, dd.y, dd.z, dd.w};
    unsigned id[4], e[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float mi = a.mi, D = a.D;
      if (AUTO) {
        const float2 r = rng[(p + k) / a.HW - f0];
        mi = r.x; D = r.y;
      }
      id[k] = enc_depth_idx(d[k], mi, D);
      e[k] = lut[id[k]];
    }
    unsigned* q = reinterpret_cast<unsigned*>(a.depth8 + 3 * p);
    q[0] = e[0] | (e[1] << 24);
    q[1] = (e[1] >> 8) | (e[2] << 16);
    q[2] = (e[2] >> 16) | (e[3] << 8);
    if (a.idx) *reinterpret_cast<unsigned*>(a.idx + p) = id[0] | (id[1] << 8) | (id[2] << 16) | (id[3] << 24);
    return;
  }
  for (int s = p; s < a.n; ++s) {                  // the tail: fewer than 4 pixels, one lane
    float mi = a.mi, D = a.D;
    if (AUTO) {
      const float2 r = rng[s / a.HW - f0];
      mi = r.x; D = r.y;
    }
    const unsigned id = enc_depth_idx(a.depth[s], mi, D), e = lut[id];
    for (int c = 0; c < 3; ++c) {
      if (a.rgb) a.rgb8[3 * s + c] = (uint8_t)enc_rgb_byte(a.rgb[3 * s + c]);
      a.depth8[3 * s + c] = (uint8_t)(e >> (8 * c));
    }
    if (a.idx) a.idx[s] = (uint8_t)id;
  }
}

static bool enc_shape_ok(int V, int H, int W) {
  return V >= 1 && H > 0 && W > 0 && (long long)V * H * W * 3 < (1ll << 31);
}
// [V x ENC_RANGE_WG x (min, max) keys]; its size is c.at, not rounded
static unsigned* carve_encode(Carver& c, int V) { return c.take<unsigned>((size_t)V * ENC_RANGE_WG * 2); }

}  // namespace lrf

extern "C" size_t lrf_encode_frames_workspace_bytes(int32_t V) {
  using namespace lrf;
  if (V < 1 || V > (1 << 24)) return 0;
  Carver c(nullptr);
  carve_encode(c, V);
  return c.at;
}

extern "C" int lrf_encode_frames(const float* rgb, const float* depth, int32_t V, int32_t H, int32_t W, const uint8_t* lut,
                                 const float* fixed_range, uint8_t* rgb8, uint8_t* depth8, uint8_t* depth_idx, float* range_out,
                                 void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_encode_frames";
  if (!enc_shape_ok(V, H, W)) return refuse(who, "need V >= 1, H, W > 0 and 3 V H W < 2^31");
  if (!depth || !lut || !depth8) return refuse(who, "null argument");
  if (!rgb != !rgb8) return refuse(who, "rgb and rgb8 go together");
  if (!fixed_range && !workspace) return refuse(who, "the automatic range needs a workspace");
  if (!fixed_range && V > (1 << 24)) return refuse(who, "need V <= 2^24 for the automatic range");
  if (misaligned(15, rgb, depth)) return refuse(who, "rgb and depth must be 16-byte aligned");
  if (misaligned(3, rgb8, depth8, depth_idx, range_out, workspace)) return refuse(who, "outputs and workspace must be 4-byte aligned");
  Carver c(workspace);
  unsigned* range = carve_encode(c, V);
  EncodeArgs a;
  memset(&a, 0, sizeof(a));
  a.rgb = rgb; a.depth = depth; a.lut = lut;
  a.rgb8 = rgb8; a.depth8 = depth8; a.idx = depth_idx; a.range_out = range_out;
  a.ws = range;
  a.HW = H * W; a.V = V;
  a.n = V * a.HW;
  if (fixed_range) { a.mi = fixed_range[0]; a.ma = fixed_range[1]; a.D = fixed_range[2]; }
  const unsigned blocks = blocks_for(a.n, ENC_PX);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (fixed_range) return launch(k_encode<false>, blocks, ENC_NT, st, a);
  LRF_TRY(launch(k_encode_range, dim3(ENC_RANGE_WG, V), ENC_NT, st, depth, a.HW, range));
  return launch(k_encode<true>, blocks, ENC_NT, st, a);
}
