// lrf_normals.inl -- per-ray surface normals from the gradient of the density feature (included by lrf_render.hip).
//
// Density function of a field: g(x) = density_feature(u(contract(x))), x field-local (world up to the world2rf shift).
//   grad_x g = Jc^T diag(2 / aabbSize) grad_u df
//   grad_u df   density_grad32: analytic, from the taps the value reads; 0 along a border-clamped axis
//   Jc          Jacobian of the L-inf contraction (utils/ray_utils.py:9-12): I for m = |x|_inf <= 1, else
//               s I + s' sign(x_k) x e_k^T with s = (2m - 1) / m^2, s' = 2 / m^3 - 2 / m^2, k = argmax |x|, so that
//               (Jc^T v)_j = s v_j + [j == k] s' sign(x_k) (x . v)
//   sample      n_i = -grad_x g(x_i) / max(|grad_x g(x_i)|, 1e-8)
//   ray         N = sum over {i: w_i > weight_thres} of w_i n_i with the weights lrf_render_fwd leaves in weight_out: the
//               samples the colour pass shades.  Not normalised, |N| <= acc; no shaded sample gives exactly (0, 0, 0).
//
//   k_density_grad  one lane per point: (feature, grad_u) of normalised coordinates.
//   k_normals       one wavefront per ray, S in 64-sample steps.  The weights of a step are one coalesced load; the ballot of
//                   w > thres decides wave-uniformly whether the step does anything at all (a trained scene shades a few
//                   percent of its samples), and only the lanes it names form x, the Jacobian and the 24 gathers.  Lanes
//                   keep their own partial sums over the steps; one butterfly (wave_sum: a fixed tree) per component at
//                   the end, lane 0 stores.  No atomics: the same bits on every run and for every batch split.
//                   blend_w / per_view / accumulate: normals[r] (+)= blend_w[r / per_view] * N_r, the scene's sum over
//                   its fields in field order without a pass of its own.
// Cited lines are relative to the reference's localTensoRF directory.
namespace lrf {

constexpr int NRM_NT = 256;                                         // 4 rays per workgroup

// density_feature32 (lrf_common.h) and its gradient with respect to the normalised coordinate u, from the same eight taps per plane
// (4 texels, 2 line taps, 8 channels): the feature is summed exactly as density_feature32 sums it (same bits); g[a] is the
// derivative of the bilinear / linear weights along axis a times the other factor, piecewise constant per cell along a.
// tap1d_g (lrf_backward.inl) is tap1d plus d(ix)/du: (size - 1) / 2 inside the lattice, 0 where the border clamps.
__device__ __forceinline__ float density_grad32(const DField& f, const float u[3], float g[3]) {
  float feat = 0.0f;
  float ds[3] = {0.0f, 0.0f, 0.0f};
  g[0] = g[1] = g[2] = 0.0f;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    int x0, x1, y0, y1, l0, l1; float tx, ty, tl;
    tap1d_g(u[MAT0[p]], f.pw[p], x0, x1, tx, ds[MAT0[p]]);       // (an axis is tapped by two planes and a line of the same
    tap1d_g(u[MAT1[p]], f.ph[p], y0, y1, ty, ds[MAT1[p]]);       // size: the same ds each time)
    tap1d_g(u[VEC[p]],  f.ll[p], l0, l1, tl, ds[VEC[p]]);
    const unsigned row0 = (unsigned)y0 * (unsigned)f.pw[p], row1 = (unsigned)y1 * (unsigned)f.pw[p];
    const unsigned o00 = (row0 + x0) * (LRF_CD * 4u), o10 = (row0 + x1) * (LRF_CD * 4u);
    const unsigned o01 = (row1 + x0) * (LRF_CD * 4u), o11 = (row1 + x1) * (LRF_CD * 4u);
    const unsigned q0 = (unsigned)l0 * (LRF_CD * 4u), q1 = (unsigned)l1 * (LRF_CD * 4u);
    const float w00 = (1.0f - tx) * (1.0f - ty), w10 = tx * (1.0f - ty);
    const float w01 = (1.0f - tx) * ty,          w11 = tx * ty;
    const float wl0 = 1.0f - tl, wl1 = tl;
    const float ux = 1.0f - tx, uy = 1.0f - ty;
    float sp = 0.0f, gx = 0.0f, gy = 0.0f, gl = 0.0f;
#pragma unroll
    for (int h = 0; h < LRF_CD / 4; ++h) {
      const float4 a = ld4b(f.dplane[p], o00 + 16 * h), b = ld4b(f.dplane[p], o10 + 16 * h);
      const float4 c = ld4b(f.dplane[p], o01 + 16 * h), d = ld4b(f.dplane[p], o11 + 16 * h);
      const float4 e = ld4b(f.dline[p], q0 + 16 * h), q = ld4b(f.dline[p], q1 + 16 * h);
#define LRF_DG_CH(m)                                                                                  \
      {                                                                                               \
        const float lv = e.m * wl0 + q.m * wl1;                                                       \
        sp += (a.m * w00 + b.m * w10 + c.m * w01 + d.m * w11) * lv;                                   \
        gx += ((b.m - a.m) * uy + (d.m - c.m) * ty) * lv;                                             \
        gy += ((c.m - a.m) * ux + (d.m - b.m) * tx) * lv;                                             \
        gl += (a.m * w00 + b.m * w10 + c.m * w01 + d.m * w11) * (q.m - e.m);                          \
      }
      LRF_DG_CH(x) LRF_DG_CH(y) LRF_DG_CH(z) LRF_DG_CH(w)
#undef LRF_DG_CH
    }
    feat += sp;
    g[MAT0[p]] += gx; g[MAT1[p]] += gy; g[VEC[p]] += gl;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] *= ds[a];
  return feat;
}

__global__ __launch_bounds__(256) void k_density_grad(DField f, const float* __restrict__ u, long long P,
                                                      float* __restrict__ grad_u, float* __restrict__ feat) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const float uu[3] = {u[(size_t)i * 3], u[(size_t)i * 3 + 1], u[(size_t)i * 3 + 2]};
  float g[3];
  const float v = density_grad32(f, uu, g);
  grad_u[(size_t)i * 3] = g[0]; grad_u[(size_t)i * 3 + 1] = g[1]; grad_u[(size_t)i * 3 + 2] = g[2];
  if (feat) feat[i] = v;
}

// unit normal of the density function at the sample with distance zk on ray (o, dh); 0 where the gradient vanishes
__device__ __forceinline__ void sample_normal(const DField& f, const float o[3], const float dh[3], float zk, float n[3]) {
  const float x[3] = {o[0] + dh[0] * zk, o[1] + dh[1] * zk, o[2] + dh[2] * zk};     // as sample_point forms it
  float xc[3] = {x[0], x[1], x[2]};
  contract3(xc[0], xc[1], xc[2]);
  float u[3], g[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) u[a] = (xc[a] - f.lo[a]) * f.inv[a] - 1.0f;
  density_grad32(f, u, g);
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] *= f.inv[a];
  contract3_bwd(x, g);                                             // Jc^T (lrf_backward.inl: the rays-gradient's own)
  const float len = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  const float r = -1.0f / fmaxf(len, 1e-8f);
  n[0] = g[0] * r; n[1] = g[1] * r; n[2] = g[2] * r;
}

__global__ __launch_bounds__(NRM_NT) void k_normals(DField f, const float* __restrict__ rays, const float* __restrict__ z,
                                                    int R, int S, const float* __restrict__ w_all,
                                                    const float* __restrict__ acc_in, const float* __restrict__ blend_w,
                                                    int per_view, int accumulate, float* __restrict__ normals,
                                                    float* __restrict__ acc_out) {
  const int lane = threadIdx.x & 63;
  const int ray = blockIdx.x * (NRM_NT / 64) + (threadIdx.x >> 6);
  if (ray >= R) return;                                             // whole waves leave: no barrier below
  const float* rp = rays + (size_t)ray * 6;
  const float o[3] = {rp[0], rp[1], rp[2]};
  const float dn = sqrtf(rp[3] * rp[3] + rp[4] * rp[4] + rp[5] * rp[5]);            // tensorBase.py:578-580
  const float dh[3] = {rp[3] / dn, rp[4] / dn, rp[5] / dn};
  const float* wr = w_all + (size_t)ray * S;
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
  for (int k0 = 0; k0 < S; k0 += 64) {
    const int k = k0 + lane;
    const float w = k < S ? wr[k] : 0.0f;
    const bool sh = k < S && w > f.weight_thres;                    // tensorBase.py:622 (a NaN weight is not shaded)
    if (__ballot(sh) == 0ull) continue;                             // wave-uniform
    if (sh) {
      float n[3];
      sample_normal(f, o, dh, z[k], n);
      a0 += w * n[0]; a1 += w * n[1]; a2 += w * n[2];
    }
  }
  a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
  if (lane == 0) {
    float a = acc_in[ray];
    if (blend_w) {
      const float bw = blend_w[ray / per_view];
      a0 *= bw; a1 *= bw; a2 *= bw; a *= bw;
    }
    float* np = normals + (size_t)ray * 3;
    if (accumulate) { a0 += np[0]; a1 += np[1]; a2 += np[2]; }
    np[0] = a0; np[1] = a1; np[2] = a2;
    if (acc_out) acc_out[ray] = accumulate ? acc_out[ray] + a : a;
  }
}

// [the forward's workspace] [weights R S] [rgb 3 R] [depth R] [acc R], every piece padded to 256 bytes
struct NormalsWs { float* w; float* rgb; float* depth; float* acc; size_t bytes; };
static NormalsWs carve_normals(void* ws, int R, int S) {
  NormalsWs n;
  Carver c(ws);
  c.take<char>(lrf_workspace_bytes(R, S), 256);
  n.w = c.take<float>((size_t)R * S, 256);
  n.rgb = c.take<float>((size_t)R * 3, 256);
  n.depth = c.take<float>(R, 256);
  n.acc = c.take<float>(R, 256);
  n.bytes = c.bytes();
  return n;
}

}  // namespace lrf

extern "C" int lrf_density_gradient(const LrfField* f, const float* u, int64_t P, float* grad_u, float* feat, void* stream) {
  using namespace lrf;
  const char* who = "lrf_density_gradient";
  if (!f || !f->cache) return refuse(who, "null argument");
  if (P < 0 || P > 256ll * 0x7fffffffll) return refuse(who, "need 0 <= P <= 256 (2^31 - 1)");
  if (P == 0) return 0;                                             // (empty arrays may be null)
  if (!u || !grad_u) return refuse(who, "null argument");
  if (misaligned(3, u, grad_u, feat)) return refuse(who, "float arrays must be 4-byte aligned");
  return launch(k_density_grad, blocks_for(P, 256), 256, reinterpret_cast<hipStream_t>(stream), make_dfield(f), u, (long long)P, grad_u, feat);
}

extern "C" size_t lrf_normals_workspace_bytes(int32_t R, int32_t S) {
  if (R <= 0 || S < 2 || S > 4096) return 0;
  return lrf::carve_normals(nullptr, R, S).bytes;
}

extern "C" int lrf_render_normals(const LrfField* f, const float* rays, const float* z, int32_t R, int32_t S, uint32_t flags,
                                  float floater_thresh, const float* blend_w, int32_t per_view, int32_t accumulate,
                                  float* normals, float* acc, void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_render_normals";
  if (!f || !f->cache || !rays || !z || !normals || !workspace) return refuse(who, "null argument");
  if (R <= 0 || S < 2 || S > 4096) return refuse(who, "need R > 0 and 2 <= S <= 4096");
  if (blend_w && per_view < 1) return refuse(who, "blend_w needs per_view >= 1");
  if (accumulate != 0 && accumulate != 1) return refuse(who, "accumulate must be 0 or 1");
  if (misaligned(3, rays, z, blend_w, normals, acc)) return refuse(who, "float arrays must be 4-byte aligned");
  if (misaligned(255, workspace)) return refuse(who, "workspace must be 256-byte aligned");
  const NormalsWs n = carve_normals(workspace, R, S);
  if (const char* bad = check_fwd(f, rays, z, n.rgb, n.depth, workspace, R, S, flags)) return refuse(bad);
  LRF_HIP(lds_opt_in());
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(render_fwd_pipelined(f, rays, z, R, S, flags, floater_thresh, n.rgb, n.depth, n.w, n.acc, workspace, st));
  return launch(k_normals, blocks_for(R, NRM_NT / 64), NRM_NT, st, make_dfield(f), rays, z, R, S, n.w, n.acc, blend_w, per_view,
                accumulate, normals, acc);
}
