// lrf_quantile.inl -- per-ray depth quantiles: the distance at which a ray's accumulated weight first reaches q (included by
// lrf_render.hip after lrf_normals.inl, whose workspace layout it shares).  q = 0.5 is the median depth.
//
// Per ray, all fp32, contraction OFF (no fused multiply-add is formed: every product and sum below is rounded on its own, so
// that a numpy restatement matches bit for bit); division and square root are IEEE:
//   inputs   w_0..w_{S-1}  the weights lrf_render_fwd leaves in weight_out (alpha mask, floater filter and term_T applied)
//            z_0..z_{S-1}  the sample distances
//            dn = sqrt((d.x d.x + d.y d.y) + d.z d.z)  k_normals' expression (tensorBase.py:578-580)
//   scan     S is walked in steps of 64 samples, lane l of step k0 holding sample k0 + l (0 beyond S).  Inside a step
//            P_l is the inclusive Hillis-Steele scan of the 64 lane values: for d = 1, 2, 4, 8, 16, 32 in this order every
//            lane l >= d replaces p_l by p_l + p_{l-d} (all lanes from the values of the round before).  Then
//              C_{k0+l} = carry + P_l       carry = 0 for the first step, C_{k0-1} (lane 63 of the step before) afterwards
//            One fixed order per ray, whatever R, K or the batch split.
//   crossing for each q_k (0 < q_k <= 1, up to 4 per call, any order): i* = the smallest i < S with C_i >= q_k -- the first
//            set lane of the ballot in the first step that has one.  The scan may be non-monotone by an ulp; "smallest i" is
//            still well defined.  None (the opacity never reaches q_k, or a NaN weight comes first: a NaN poisons every
//            later C and no comparison with it holds): depth exactly 0.0f, index -1 -- what lrf_points_fuse, backproject and
//            lrf_tsdf_integrate treat as "no depth".
//   depth    t = min(max((q_k - C_{i*-1}) / w_{i*}, 0), 1) with C_{-1} = 0 and C_{i*-1} the scan's own value (never
//            C_{i*} - w_{i*});  depth = (z_{i*} + t (z_{i*+1} - z_{i*})) / dn, z_{i*+1} := z_{i*} for i* = S - 1:
//            linear interpolation in accumulated weight inside the crossing sample's interval.
//   finish   lane 0, with blend_w / per_view / accumulate as lrf_render_normals means them (bw = blend_w[r / per_view]):
//              depth[k, r] (+)= bw depth  when found (adds nothing otherwise),  wsum[k, r] (+)= bw [found],  acc[r] (+)= bw acc
//            without blend_w: depth[k, r] = depth, wsum[k, r] = [found], acc[r] = acc.  A scene divides depth by wsum at the
//            end, so a field without a crossing does not drag a pixel towards zero.
//
//   k_depth_quantiles  one wavefront per ray.  A step's weights are one coalesced load, the scan runs in registers through
//                      cross-lane moves, and the wave leaves its loop (wave-uniformly) once all K quantiles are found: a
//                      trained scene crosses 0.5 within its first few steps.  No LDS, no atomics, no barrier; whole waves
//                      return on ray >= R.  acc comes from the forward's acc_out, not from this pass.
// Cited lines are relative to the reference's localTensoRF directory.
namespace lrf {

constexpr int QNT_NT = 256;                                         // 4 rays per workgroup
constexpr int QNT_MAXK = 4;

struct QuantileQ { float q[QNT_MAXK]; int K; };

__global__ __launch_bounds__(QNT_NT) void k_depth_quantiles(const float* __restrict__ rays, const float* __restrict__ z, int R, int S,
                                                            const float* __restrict__ w_all, const float* __restrict__ acc_in,
                                                            QuantileQ qs, const float* __restrict__ blend_w, int per_view,
                                                            int accumulate, float* __restrict__ depth, float* __restrict__ wsum,
                                                            int* __restrict__ index, float* __restrict__ acc_out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * (QNT_NT / 64) + (threadIdx.x >> 6);
  if (ray >= R) return;                                             // whole waves leave: no barrier below
  const float* wr = w_all + (size_t)ray * S;
  int idx[QNT_MAXK];
  float cprev[QNT_MAXK], wx[QNT_MAXK];
#pragma unroll
  for (int j = 0; j < QNT_MAXK; ++j) { idx[j] = -1; cprev[j] = 0.0f; wx[j] = 1.0f; }
  unsigned pending = (1u << qs.K) - 1u;                             // wave-uniform throughout
  float carry = 0.0f;
  for (int k0 = 0; k0 < S && pending; k0 += 64) {
    const int k = k0 + lane;
    const float w = k < S ? wr[k] : 0.0f;
    float p = w;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float t = __shfl_up(p, d, 64);
      if (lane >= d) p = p + t;
    }
    const float c = carry + p;
    float prev = __shfl_up(c, 1, 64);
    if (lane == 0) prev = carry;
#pragma unroll
    for (int j = 0; j < QNT_MAXK; ++j) {
      if (!((pending >> j) & 1u)) continue;
      const unsigned long long m = __ballot(k < S && c >= qs.q[j]);
      if (m == 0ull) continue;                                      // wave-uniform
      const int first = __ffsll((long long)m) - 1;
      idx[j] = k0 + first;
      cprev[j] = __shfl(prev, first, 64);
      wx[j] = __shfl(w, first, 64);
      pending &= ~(1u << j);
    }
    carry = __shfl(c, 63, 64);
  }
  if (lane != 0) return;
  const float* rp = rays + (size_t)ray * 6;
  const float dn = sqrtf((rp[3] * rp[3] + rp[4] * rp[4]) + rp[5] * rp[5]);          // tensorBase.py:578-580
  const float bw = blend_w ? blend_w[ray / per_view] : 1.0f;
#pragma unroll
  for (int j = 0; j < QNT_MAXK; ++j) {
    if (j >= qs.K) break;
    const bool found = idx[j] >= 0;
    float d = 0.0f;
    if (found) {
      const float t = fminf(fmaxf((qs.q[j] - cprev[j]) / wx[j], 0.0f), 1.0f);
      const float z0 = z[idx[j]], z1 = z[idx[j] + 1 < S ? idx[j] + 1 : idx[j]];
      d = (z0 + t * (z1 - z0)) / dn;
      if (blend_w) d = bw * d;
    }
    const float ws = found ? bw : 0.0f;
    const size_t o = (size_t)j * R + ray;
    depth[o] = accumulate ? depth[o] + d : d;
    if (wsum) wsum[o] = accumulate ? wsum[o] + ws : ws;
    if (index) index[o] = idx[j];
  }
  if (acc_out) {
    float a = acc_in[ray];
    if (blend_w) a = bw * a;
    acc_out[ray] = accumulate ? acc_out[ray] + a : a;
  }
}

// the requested quantiles as the kernel's by-value argument; false when one is outside (0, 1] or NaN
static bool quantile_args(const float* q, int32_t K, QuantileQ& qs) {
  qs.K = K;
  for (int j = 0; j < QNT_MAXK; ++j) {
    qs.q[j] = j < K ? q[j] : 1.0f;
    if (j < K && !(q[j] > 0.0f && q[j] <= 1.0f)) return false;
  }
  return true;
}

static int launch_quantiles(const float* rays, const float* z, int R, int S, const float* w, const float* acc_in,
                            const QuantileQ& qs, const float* blend_w, int per_view, int accumulate, float* depth, float* wsum,
                            int32_t* index, float* acc, hipStream_t st) {
  return launch(k_depth_quantiles, blocks_for(R, QNT_NT / 64), QNT_NT, st, rays, z, R, S, w, acc_in, qs, blend_w, per_view, accumulate,
                depth, wsum, index, acc);
}

// what the two entry points refuse alike; leaves the quantiles in qs
static int quantile_shape(const char* who, int R, int S, const float* q, int K, QuantileQ& qs) {
  if (R <= 0 || S < 2 || S > 4096) return refuse(who, "need R > 0 and 2 <= S <= 4096");
  if (K < 1 || K > QNT_MAXK) return refuse(who, "need 1 <= K <= 4 quantiles");
  if (!quantile_args(q, K, qs)) return refuse(who, "every q must lie in (0, 1]");
  return 0;
}

}  // namespace lrf

extern "C" size_t lrf_quantile_workspace_bytes(int32_t R, int32_t S) {
  if (R <= 0 || S < 2 || S > 4096) return 0;
  return lrf::carve_normals(nullptr, R, S).bytes;                   // the forward's workspace, the [R,S] weights, 5 R floats
}

extern "C" int lrf_render_depth_quantiles(const LrfField* f, const float* rays, const float* z, int32_t R, int32_t S, uint32_t flags,
                                          float floater_thresh, const float* q, int32_t K, const float* blend_w, int32_t per_view,
                                          int32_t accumulate, float* depth, float* wsum, int32_t* index, float* acc,
                                          void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_render_depth_quantiles";
  if (!f || !f->cache || !rays || !z || !q || !depth || !workspace) return refuse(who, "null argument");
  QuantileQ qs;
  LRF_TRY(quantile_shape(who, R, S, q, K, qs));
  if (blend_w && per_view < 1) return refuse(who, "blend_w needs per_view >= 1");
  if (accumulate != 0 && accumulate != 1) return refuse(who, "accumulate must be 0 or 1");
  if (accumulate && index) return refuse(who, "an index cannot be accumulated (accumulate = 1 needs index = NULL)");
  if (blend_w && !wsum) return refuse(who, "blend_w needs wsum (the divisor of the blended depth)");
  if (misaligned(3, rays, z, blend_w, depth, wsum, index, acc)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  if (misaligned(255, workspace)) return refuse(who, "workspace must be 256-byte aligned");
  const NormalsWs n = carve_normals(workspace, R, S);
  if (const char* bad = check_fwd(f, rays, z, n.rgb, n.depth, workspace, R, S, flags)) return refuse(bad);
  LRF_HIP(lds_opt_in());
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(render_fwd_pipelined(f, rays, z, R, S, flags, floater_thresh, n.rgb, n.depth, n.w, n.acc, workspace, st));
  return launch_quantiles(rays, z, R, S, n.w, n.acc, qs, blend_w, per_view, accumulate, depth, wsum, index, acc, st);
}

// the kernel alone on caller-supplied weights (include/lrf_debug.h)
extern "C" int lrf_depth_quantiles_from_weights(const float* w, const float* z, const float* rays, int32_t R, int32_t S, const float* q,
                                                int32_t K, float* depth, int32_t* index, void* stream) {
  using namespace lrf;
  const char* who = "lrf_depth_quantiles_from_weights";
  if (!w || !z || !rays || !q || !depth) return refuse(who, "null argument");
  QuantileQ qs;
  LRF_TRY(quantile_shape(who, R, S, q, K, qs));
  if (misaligned(3, w, z, rays, depth, index)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  return launch_quantiles(rays, z, R, S, w, nullptr, qs, nullptr, 1, 0, depth, nullptr, index, nullptr, reinterpret_cast<hipStream_t>(stream));
}
