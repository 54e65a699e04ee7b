// lrf_render.hip -- gfx950 (MI355X / CDNA4) forward kernels of the localrf render path and the C ABI declared in
// include/lrf.h.  One translation unit (this file + the .inl files it includes), built without the SLP vectoriser
// (lrf_tu.h says why).  In include order: lrf_common.h, lrf_host.inl (the host helpers of every entry point: refuse, launch,
// misaligned, Carver, TwoStreams), lrf_tiles.inl, lrf_shade3.inl (+ lrf_shade3_kernel.inl), lrf_generic.inl, lrf_forward.inl (the
// forward's host side: workspace, launch plan and helpers, lrf_render_fwd), lrf_backward.inl (+ lrf_train32.inl), lds_opt_in
// (behind every kernel it names), lrf_scene / adam / losses / metrics / frames / select / evalgeo / encode .inl, lrf_compact.inl
// and the geometry files (lrf_points, lrf_mesh, lrf_mesh_clean / simplify / smooth / raster / texture / distance,
// lrf_tsdf_blocks), lrf_reg.inl, lrf_mask.inl, lrf_normals.inl, lrf_quantile.inl; this file keeps the kernels, the debug
// setters and the small feature / sampling / pack entry points.
//
// Pipeline of lrf_render_fwd (one field, R rays x S samples), two launches, no atomics on floats:
//   k_march      one wavefront per ray: contracted sampling, density VM gather (channel-last planes, 2 x float4 per tap,
//                lines staged in LDS), softplus, alpha, wave-level prefix product for transmittance, acc / depth,
//                floater filter, and in-wave compaction of the samples that pass weight > thres into the ray's list
//                (u16 index + weight); also leaves d / |d| per ray for the colour kernel.
//   k_shade3     (lrf_shade3.inl) the colour stage, 32 samples per wave on v_mfma_f32_32x32x16_bf16: tile scan,
//                appearance gather, basis -> 128 -> 128 as a register-resident split-bf16 MFMA chain, VALU head,
//                per-ray ordered sum of the tile partials + white background.
// Other colour engines behind the same ABI: k_shade (exact fp32 on v_mfma_f32_16x16x4_f32, LRF_FLAG_MLP_F32) and
// k_shade_gen (lrf_generic.inl: fp32 tile GEMMs on the vector ALU -- LRF_FLAG_MLP_VALU, and every colour-network configuration
// other than opt.py's defaults), both behind k_finalize.
// The split-bf16 helpers of the 16-sample chain (gemm_step ...) serve the training kernels of lrf_backward.inl.
//
// Reference lines (relative to /root/reference/localTensoRF) are cited at each step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <mutex>
#include "lrf_common.h"
#include "lrf_host.inl"

namespace lrf {

constexpr int ITEM = 16;          // compact samples per shade work item = one 16-column MFMA tile

thread_local char g_err[512] = "";       // one error text per thread for the whole library (lrf_error_slot; written by refuse, lrf_host.inl)

// ---------------------------------------------------------------------------- pack
// [C,H,W] -> [H,W,CS] channel-last; app=1: padded appearance layout (slot app_pc(c), zero pads)
struct PackSeg { const float* src; float* dst; int C, H, W, CS, app; };
struct PackTab { PackSeg s[18]; };
struct PackMlp { float* mlp; uint32_t* mlpb; uint32_t* mlpw; uint32_t* mlpwt; int mode; };   // mode 0: all four network images; 1: generic engine (only the basis^T fragments of mlpwt)
__device__ void pack_mlp_elem(const LrfParams& p, float* __restrict__ img, int idx);
__device__ void pack_mlp_bf16_elem(const LrfParams& p, uint32_t* __restrict__ img, int idx);
__device__ void pack_mlp_w32_elem(const LrfParams& p, uint32_t* __restrict__ img, int idx);
__device__ void pack_mlp_w32_t_elem(const LrfParams& p, uint32_t* __restrict__ img, int idx, int basis_only);
// The whole layout cache in ONE launch: all plane / line tensors of a field (the appearance ones twice: padded and dense;
// blockIdx.z < 18 selects; a line [C,L,1] is a plane with H = 1) and, in slice 18, the four fragment-ordered images of the
// colour network (they were four launches of ~5 us each, three of them in front of every training forward).
__global__ __launch_bounds__(128) void k_pack_planes(PackTab tab, LrfParams p, PackMlp pm, int z0 /* first slice of this launch: 0, or 18 = the network images only (lrf_adam_step_pack) */) {
  const int zsl = (int)blockIdx.z + z0;
  if (zsl == 18) {
    const int nthr = gridDim.x * gridDim.y * 128;
    for (int idx = (blockIdx.y * gridDim.x + blockIdx.x) * 128 + threadIdx.x; idx < 26880; idx += nthr) {   // >= the largest image (IMGB_ALL * 4 = 26624)
      if (pm.mode == 0) {
        pack_mlp_elem(p, pm.mlp, idx);
        pack_mlp_bf16_elem(p, pm.mlpb, idx);
        pack_mlp_w32_elem(p, pm.mlpw, idx);
      }
      pack_mlp_w32_t_elem(p, pm.mlpwt, idx, pm.mode);
    }
    return;
  }
  const PackSeg sg = tab.s[zsl];
  const float* __restrict__ src = sg.src;
  float* __restrict__ dst = sg.dst;
  const int C = sg.C, H = sg.H, W = sg.W, CS = sg.CS, app = sg.app;
  if ((int)blockIdx.y >= H) return;
  // a block packs 128 consecutive texels of one row: channel rows are read 128 floats at a time into LDS, the
  // CS-float records of those texels are one contiguous span of the destination and leave as float4 (a thread writing
  // its own record dword by dword stored 4 bytes at a 32- or 128-byte stride)
  __shared__ __attribute__((aligned(16))) float s_t[128 * (LRF_CAS + 4)];
  const int x0 = blockIdx.x * 128, y = blockIdx.y, t = threadIdx.x;
  if (x0 >= W) return;
  const int nx = min(128, W - x0);
  const int ld = CS + 4;                                    // records stay 16-byte aligned in LDS
  if (t < nx) {
    float* d = &s_t[t * ld];
    if (app) for (int q = 0; q < 4; ++q) { d[8 * q + 6] = 0.0f; d[8 * q + 7] = 0.0f; }
    for (int c = 0; c < C; ++c) d[app ? app_pc(c) : c] = src[((size_t)c * H + y) * W + x0 + t];
  }
  __syncthreads();
  float4* out = reinterpret_cast<float4*>(dst + ((size_t)y * W + x0) * CS);
  const int q4 = CS / 4, n4 = nx * q4;
  for (int i = t; i < n4; i += 128) out[i] = *reinterpret_cast<const float4*>(&s_t[(i / q4) * ld + 4 * (i % q4)]);
}
// colour network -> MFMA-fragment-ordered image (see lrf_common.h IMG_*).
// Fragment lane l = (i = l & 15, g = l >> 4): A operand row 16t'+i, K-slot g.
__device__ void pack_mlp_elem(const LrfParams& p, float* __restrict__ img, int idx) {
  if (idx >= IMG_FLOATS) return;
  float v = 0.0f;
  if (idx < IMG_W1) {                       // basis_mat.weight [27,72]   (tensoRF.py:25-27,196)
    const int e = idx - IMG_BAS;
    const int j = e & 7, lane = (e >> 3) & 63, tp = e >> 9;          // tp = t'*3 + p
    const int t1 = tp / 3, pl = tp % 3;
    const int row = 16 * t1 + (lane & 15), col = pl * LRF_CA + 6 * (lane >> 4) + j;
    if (row < LRF_APP_DIM && j < 6) v = p.basis[row * 72 + col];
  } else if (idx < IMG_W2) {                // mlp.0.weight [128,27]      (tensorBase.py:105)
    const int e = idx - IMG_W1;
    const int r = e & 3, lane = (e >> 2) & 63, tt = e >> 8;            // tt = t'*2 + t
    const int t1 = tt >> 1, t0 = tt & 1;
    const int row = 16 * t1 + (lane & 15), col = 16 * t0 + 4 * (lane >> 4) + r;
    if (col < LRF_APP_DIM) v = p.w1[row * LRF_APP_DIM + col];
  } else if (idx < IMG_W3H) {               // mlp.2.weight [128,128]     (tensorBase.py:106)
    const int e = idx - IMG_W2;
    const int r = e & 3, lane = (e >> 2) & 63, tt = e >> 8;            // tt = t'*8 + t
    const int t1 = tt >> 3, t0 = tt & 7;
    const int row = 16 * t1 + (lane & 15), col = 16 * t0 + 4 * (lane >> 4) + r;
    v = p.w2[row * LRF_FEATC + col];
  } else if (idx < IMG_B1) {                // mlp_view.0.weight[:, :128] (tensorBase.py:107)
    const int e = idx - IMG_W3H;
    const int o = e & 3, fidx = (e >> 2) & 31, g = e >> 7;
    const int feat = 16 * (fidx >> 2) + 4 * g + (fidx & 3);
    if (o < 3) v = p.w3[o * (LRF_FEATC + 3) + feat];
  } else if (idx < IMG_B2) {
    v = p.b1[idx - IMG_B1];
  } else if (idx < IMG_W3V) {
    v = p.b2[idx - IMG_B2];
  } else {                                  // view columns + bias of mlp_view.0
    const int e = idx - IMG_W3V;
    const int o = e >> 2, c = e & 3;
    if (o < 3) v = (c < 3) ? p.w3[o * (LRF_FEATC + 3) + LRF_FEATC + c] : p.b3[o];
  }
  img[idx] = v;
}

__device__ __forceinline__ unsigned short bf16_bits(float v) {
  return __builtin_bit_cast(unsigned short, (__bf16)v);       // round-to-nearest-even
}
__device__ __forceinline__ float bf16_val(unsigned short b) {
  return __uint_as_float(((unsigned)b) << 16);
}

// colour network -> split-bf16 fragment image (lrf_common.h IMGB_*).  One thread per
// 32-bit word (two bf16) of the fragment area, then the fp32 tail.
__device__ void pack_mlp_bf16_elem(const LrfParams& p, uint32_t* __restrict__ img, int idx) {
  if (idx >= IMGB_ALL * 4) return;
  if (idx >= IMGB_W3F * 4) {                                   // head fragments (k_mlp): frag = ks
    const int e = idx - IMGB_W3F * 4;
    const int u4 = e >> 2, wj = e & 3;
    const int lane = u4 & 63, part = (u4 >> 6) & 1, ks = u4 >> 7;
    const int i = lane & 15, g = lane >> 4;
    unsigned short out[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * wj + h;
      const int col = 16 * (2 * ks + (j >> 2)) + 4 * g + (j & 3);
      const float v = i < 3 ? p.w3[i * (LRF_FEATC + 3) + col] : 0.0f;
      const unsigned short hi = bf16_bits(v);
      out[h] = part ? bf16_bits(v - bf16_val(hi)) : hi;
    }
    img[idx] = (uint32_t)out[0] | ((uint32_t)out[1] << 16);
    return;
  }
  if (idx >= IMGB_TAIL * 4) {                                  // fp32 tail
    const int e = idx - IMGB_TAIL * 4;
    float v = 0.0f;
    if (e < TAIL_B1) {
      const int g = e / TAIL_W3H_GS, rem = e % TAIL_W3H_GS;
      const int o = rem & 3, fidx = rem >> 2;
      const int feat = 16 * (fidx >> 2) + 4 * g + (fidx & 3);
      if (o < 3 && fidx < 32) v = p.w3[o * (LRF_FEATC + 3) + feat];
    } else if (e < TAIL_B2) v = p.b1[e - TAIL_B1];
    else if (e < TAIL_W3V) v = p.b2[e - TAIL_B2];
    else {
      const int o = (e - TAIL_W3V) >> 2, c = (e - TAIL_W3V) & 3;
      if (o < 3) v = (c < 3) ? p.w3[o * (LRF_FEATC + 3) + LRF_FEATC + c] : p.b3[o];
    }
    img[idx] = __float_as_uint(v);
    return;
  }
  // word -> (frag, part, lane, j pair)
  const int u4 = idx >> 2, wj = idx & 3;
  const int lane = u4 & 63, part = (u4 >> 6) & 1, frag = u4 >> 7;
  const int i = lane & 15, g = lane >> 4;
  unsigned short out[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int j = 2 * wj + h;
    float v = 0.0f;
    if (frag < 6) {                                            // basis: frag = t'*3 + ks
      const int t1 = frag / 3, pl = frag % 3, row = 16 * t1 + i;
      if (j < 6 && row < LRF_APP_DIM) v = p.basis[row * 72 + pl * LRF_CA + 6 * g + j];
    } else if (frag < 14) {                                    // layer 1: frag-6 = t'
      const int t1 = frag - 6;
      const int col = 16 * (j >> 2) + 4 * g + (j & 3);
      if (col < LRF_APP_DIM) v = p.w1[(16 * t1 + i) * LRF_APP_DIM + col];
    } else {                                                   // layer 2: frag-14 = t'*4 + ks
      const int t1 = (frag - 14) >> 2, ks = (frag - 14) & 3;
      const int col = 16 * (2 * ks + (j >> 2)) + 4 * g + (j & 3);
      v = p.w2[(16 * t1 + i) * LRF_FEATC + col];
    }
    const unsigned short hi = bf16_bits(v);
    out[h] = part ? bf16_bits(v - bf16_val(hi)) : hi;
  }
  img[idx] = (uint32_t)out[0] | ((uint32_t)out[1] << 16);
}

// colour network -> w32 fragment image (lrf_common.h W32_*), for k_shade3.  One thread per 32-bit word.
__device__ void pack_mlp_w32_elem(const LrfParams& p, uint32_t* __restrict__ img, int idx) {
  if (idx >= W32_ALL_U4 * 4) return;
  if (idx >= W32_U4 * 4) {                                     // fp32 tail
    const int e = idx - W32_U4 * 4;
    float v = 0.0f;
    if (e < W32_T_B2) v = p.b1[e - W32_T_B1];
    else if (e < W32_T_W3) v = p.b2[e - W32_T_B2];
    else if (e < W32_T_B3) {
      const int c = (e - W32_T_W3) / W32_T_W3_LD, u = (e - W32_T_W3) % W32_T_W3_LD;
      if (u < LRF_FEATC + 3) v = p.w3[c * (LRF_FEATC + 3) + u];
    } else if (e < W32_T_B3 + 3) v = p.b3[e - W32_T_B3];
    img[idx] = __float_as_uint(v);
    return;
  }
  const int u4 = idx >> 2, wj = idx & 3;
  const int lane = u4 & 63, part = (u4 >> 6) & 1, frag = u4 >> 7;
  const int n = lane & 31, h = lane >> 5;
  unsigned short out[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const int j = 2 * wj + hh;
    float v = 0.0f;
    if (frag < W32_W1) {                                       // basis_mat.weight [27,72] (tensoRF.py:25-27,196)
      const int c = w32_chan(h, 8 * frag + j);
      if (c >= 0 && n < LRF_APP_DIM) v = p.basis[n * 72 + c];
    } else if (frag < W32_W2) {                                // mlp.0.weight [128,27] (tensorBase.py:105)
      const int e = frag - W32_W1, m = e >> 1, q = e & 1;
      const int u = w32_unit(0, q, h, j);
      if (u < LRF_APP_DIM) v = p.w1[(32 * m + n) * LRF_APP_DIM + u];
    } else {                                                   // mlp.2.weight [128,128] (tensorBase.py:106)
      const int e = frag - W32_W2, m = e >> 3, m0 = (e >> 1) & 3, q = e & 1;
      v = p.w2[(32 * m + n) * LRF_FEATC + w32_unit(m0, q, h, j)];
    }
    const unsigned short hi = bf16_bits(v);
    out[hh] = part ? bf16_bits(v - bf16_val(hi)) : hi;
  }
  img[idx] = (uint32_t)out[0] | ((uint32_t)out[1] << 16);
}

// --------------------------------------------------------------------------- march
// One wavefront per ray.  tensorBase.py:576-622 (sampling, density, alpha2weights,
// acc/depth, floater filter, shading mask).
// LDSL: the three density lines ([L][8] floats each, 9.6 KB at 300) are staged in LDS behind the per-wave alpha
// slices, so a sample costs 24 texture-path loads instead of 36 (the march is bound by that path: TA 57 % busy)
// Several fields in one launch (LocalTensorfs' blended evaluation, local_tensorfs.py:440-474: every active field renders
// every ray): the rays of the fields are one list of nf * Rf "virtual" rays, field-major -- exactly the layout of
// lrf_scene_rays' [n_rf, R, 6] output -- and a workgroup / a tile range picks its field's DField.  All per-ray arrays
// (counts, compaction lists, partials, unit directions, outputs) are indexed by the virtual ray.
constexpr int LRF_MULTI_MAX = 4;
// Rs / lo: a chunk of a larger batch -- the rays the caller sees (inputs `rays`, outputs `rgb`, `depth`) of field k's r-th ray of
// the chunk sit at index k * Rs + lo + r of arrays laid out [n_rf][Rs]; Rs = Rf, lo = 0 when the chunk is the batch.
struct MultiF { DField f[LRF_MULTI_MAX]; int nf, Rf, Rs, lo; };
__device__ __forceinline__ int multi_io(const MultiF& m, int k, int vray) { return k * m.Rs + m.lo + (vray - k * m.Rf); }
template <bool MULTI> struct FieldArg { typedef DField type; };
template <> struct FieldArg<true> { typedef MultiF type; };
__device__ __forceinline__ const DField& field_of(const DField& f, int) { return f; }
__device__ __forceinline__ const DField& field_of(const MultiF& m, int k) { return m.f[k]; }

// Pass B runs the in-chunk scans of MARCH_G chunks together (see there).
constexpr int MARCH_G = 8;
constexpr int MARCH_SR = 3;         // rounds of the line staging whose loads are issued together
constexpr int MARCH_LDS_TAIL = 16;  // bytes of dynamic LDS behind alpha slices, lines and z: the combine word of gsum
constexpr int MARCH_TILE = 32;      // samples per tile of the colour kernel (ITEM3, lrf_shade3.inl): the unit of gsum
// TIMED (debug, lrf_debug_march_phases): __builtin_readcyclecounter() totals per wave -> dump[ray][4] = {line / z staging
// with its barrier, pass A, pass B, epilogue}; the production kernels carry none of it.
// ZLDS: the sample schedule z[0..S) sits in LDS behind the lines (it is the same 4 * S bytes for every ray: pass A read
// z[k] and z[k + 1] and pass B z[k] again per lane through the vector-memory path); launch_march decides.
template <bool LDSL, bool MULTI, bool TIMED>
__device__ __forceinline__ void march_body(
    const typename FieldArg<MULTI>::type& fin, const float* __restrict__ rays, const float* __restrict__ z, int R, int S,
    uint32_t flags, float floater,
    float* __restrict__ depth, float* __restrict__ acc_ws, float* __restrict__ w_all,
    int* __restrict__ ncomp, int* __restrict__ gsum, uint16_t* __restrict__ cidx, float* __restrict__ cw,
    float* __restrict__ feat_out, const bool zlds) {
  extern __shared__ float s_alpha_all[];
  unsigned long long tk[4] = {0, 0, 0, 0}, tlast = 0;
#define LRF_MTICK(i) do { if (TIMED) { const unsigned long long now_ = __builtin_readcyclecounter(); tk[i] += now_ - tlast; tlast = now_; } } while (0)
  if (TIMED) tlast = __builtin_readcyclecounter();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nb = gridDim.x;                              // XCD-aware block order, see tile_walk_begin
  const int lb = (nb % 8 == 0) ? (int)(blockIdx.x % 8) * (nb / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const int nw = blockDim.x >> 6;                          // rays per workgroup: 4, 8 or 16 (launch_march)
  const int ray = lb * nw + wave;
  int fk_ = 0;
  if constexpr (MULTI) fk_ = min((lb * nw) / fin.Rf, fin.nf - 1);   // the workgroup's field (Rf is a multiple of nw: one field per workgroup)
  const DField& f = field_of(fin, fk_);
  int io_ray = ray;                                        // where the caller keeps this ray (rays in, depth out)
  if constexpr (MULTI) io_ray = multi_io(fin, fk_, ray);
  const float* s_line[3] = {nullptr, nullptr, nullptr};
  float* s_z = s_alpha_all + (size_t)nw * S;               // the schedule, behind the alpha slices and the lines
  const int zi0 = threadIdx.x, zi1 = threadIdx.x + blockDim.x;
  float z0 = 0.0f, z1 = 0.0f;                              // its first two rounds are loaded here, in flight under the line loads
  if (zlds && zi0 < S) z0 = z[zi0];
  if (zlds && zi1 < S) z1 = z[zi1];
  if (LDSL) {                                              // lines behind the alpha slices (whole block: before any return)
    // All loads of a thread's share first, then the LDS stores: MARCH_SR rounds of the three lines are 3 * MARCH_SR
    // independent loads in flight (branch-free: a clamped index, the store is what is predicated).  Line by line and
    // round by round, as this was, each load was waited for before the next one was issued -- nine memory latencies in
    // a row in front of the barrier at 300^3 (the phase clocks: 6.8 K of a wave's 92 K cycles).
    float* base = s_alpha_all + (size_t)nw * S;
    float4* dst[3]; const float4* src[3]; int n[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      n[p] = f.ll[p] * LRF_CD / 4;
      dst[p] = reinterpret_cast<float4*>(base);
      src[p] = reinterpret_cast<const float4*>(f.dline[p]);
      s_line[p] = base;
      base += f.ll[p] * LRF_CD;
    }
    s_z = base;
    const int nmax = max(n[0], max(n[1], n[2])), bd = blockDim.x;
    for (int i0 = threadIdx.x; i0 < nmax; i0 += MARCH_SR * bd) {
      float4 v[3][MARCH_SR];
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int r = 0; r < MARCH_SR; ++r) v[p][r] = src[p][min(i0 + r * bd, n[p] - 1)];
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int r = 0; r < MARCH_SR; ++r) {               // (keeps the compiler from sinking each load into its predicated store)
          asm volatile("" : "+v"(v[p][r].x), "+v"(v[p][r].y), "+v"(v[p][r].z), "+v"(v[p][r].w));
          if (i0 + r * bd < n[p]) dst[p][i0 + r * bd] = v[p][r];
        }
    }
  }
  if (zlds) {
    if (zi0 < S) s_z[zi0] = z0;
    if (zi1 < S) s_z[zi1] = z1;
    for (int i = zi1 + blockDim.x; i < S; i += blockDim.x) s_z[i] = z[i];
  }
  // the workgroup's tile total (gsum): waves done << 20 | 32-sample tiles, in the 16 bytes launch_march adds behind everything
  // else (a static __shared__ word would move the dynamic part off its 16-byte alignment: the lines are read as float4)
  unsigned* s_gcomb = reinterpret_cast<unsigned*>(s_z + (zlds ? S : 0));
  if (gsum && threadIdx.x == 0) *s_gcomb = 0u;
  if (LDSL || zlds || gsum) __syncthreads();
  LRF_MTICK(0);
  if (ray >= R) return;
  float* s_alpha = s_alpha_all + (size_t)wave * S;
  const int oray = f.perm ? f.perm[ray] : io_ray;          // where the caller sees this ray (ray sorting / a chunk of a multi-field batch)

  const float* rp = rays + (size_t)io_ray * 6;
  const float o[3] = {rp[0], rp[1], rp[2]};
  const float dn = sqrtf(rp[3] * rp[3] + rp[4] * rp[4] + rp[5] * rp[5]);      // :578-580
  const float dh[3] = {rp[3] / dn, rp[4] / dn, rp[5] / dn};
  const bool relu = flags & LRF_FLAG_RELU_DENS;
  const int nchunk = (S + 63) >> 6;

  // pass A: alpha per sample -> LDS.
  //
  // Early termination: `carry` is the transmittance entering the next 64-sample chunk (a wave-level
  // product of this chunk's 1 - alpha + 1e-10, the same value in every lane).  Once it is below
  // f.term_T no later sample can pass weight > weight_thres (w_k = alpha_k T_k <= T_k <= carry), so the
  // remaining density gathers are skipped and those samples count as empty (alpha = 0, feature "not
  // evaluated"): exactly what the reference computes for a field that is empty behind that point --
  // the forced last sample (:24) picks up the remaining transmittance.  acc is unchanged; sum(w z)
  // moves by at most carry * z[S-1] (term_T = 1e-9, z <= 1000.1: 1e-6 absolute against depth * |d| >= 0.1).
  // term_T = 0 disables it.
  {
    float carry = 1.0f;
    bool live = true;                                      // wave-uniform
    for (int c = 0; c < nchunk; ++c) {
      const int k = (c << 6) + lane;
      float alpha = 0.0f, fk = -INFINITY;
      if (live && k < S - 1) {                             // last sample is never valid (:600)
        const float zk = zlds ? s_z[k] : z[k];
        float x[3], u[3];
        sample_point(f, o, dh, zk, x, u);
        bool valid = true;
        if (f.alpha_vol) valid = alpha_mask_sample(f, x[0], x[1], x[2]) > 0.0f;   // :593-598
        if (valid) {
          fk = density_feature_m<LDSL>(f, u, s_line);
          const float sigma = feature2density(fk, f.density_shift, relu);            // :603-608
          const float dist = (zlds ? s_z[k + 1] : z[k + 1]) - zk;                    // :584-587
          alpha = 1.0f - expf(-sigma * dist * f.distance_scale);                     // :610
        }
      }
      if (k < S) {
        s_alpha[k] = alpha;
        if (feat_out) feat_out[(size_t)ray * S + k] = fk;
      }
      if (live && f.term_T > 0.0f) {
        float v = (k < S - 1) ? (1.0f - alpha + 1e-10f) : 1.0f;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v *= __shfl_xor(v, d, 64);
        carry *= v;
        if (__builtin_amdgcn_readfirstlane(__float_as_int(carry)) < __float_as_int(f.term_T)) live = false;
      }
    }
  }
  // (each wave only touches its own LDS slice: no barrier needed, LDS ops are in order per wave)
  LRF_MTICK(1);

  // pass B: transmittance, weights, compaction.  Only `carry` links the 64-sample chunks of a ray; the scan inside a chunk
  // (wave_scan_prod: eight dependent cross-lane round trips) does not depend on it.  So the chunks are taken MARCH_G at a
  // time: step one reads their alphas and runs their MARCH_G shuffle ladders side by side (step d of every chunk before
  // step 2d: the round trips overlap instead of queueing), step two walks them in order with `carry` as before.  Per chunk
  // the arithmetic is wave_scan_prod's, product for product, so every output keeps its bits.
  float acc = 0.0f, dsum = 0.0f, kbar = 0.0f;
  int nsh = 0;
  const int npass = floater > 0.0f ? 2 : 1;
  for (int pass = 0; pass < npass; ++pass) {
    const bool emit = (pass == npass - 1);
    float carry = 1.0f, a_acc = 0.0f, a_d = 0.0f, a_k = 0.0f;
    for (int c0 = 0; c0 < nchunk; c0 += MARCH_G) {
      float al[MARCH_G], p[MARCH_G], ex[MARCH_G];
#pragma unroll
      for (int j = 0; j < MARCH_G; ++j) {                  // (chunks past the last one: k >= S, a scan of ones)
        const int k = ((c0 + j) << 6) + lane;
        float alpha = 0.0f;
        if (k < S) {
          alpha = s_alpha[k];
          if (pass == 1 && (float)k < kbar * floater) alpha = 0.0f;                  // :617-619
          if (k == S - 1) alpha = 1.0f;                                               // :24
        }
        al[j] = alpha;
        p[j] = (k < S) ? (1.0f - alpha + 1e-10f) : 1.0f;                              // :25-29
      }
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        float t[MARCH_G];
#pragma unroll
        for (int j = 0; j < MARCH_G; ++j) t[j] = __shfl_up(p[j], d, 64);
#pragma unroll
        for (int j = 0; j < MARCH_G; ++j) if (lane >= d) p[j] *= t[j];
      }
#pragma unroll
      for (int j = 0; j < MARCH_G; ++j) {
        ex[j] = __shfl_up(p[j], 1, 64);
        if (lane == 0) ex[j] = 1.0f;
      }
#pragma unroll
      for (int j = 0; j < MARCH_G; ++j) p[j] = __shfl(p[j], 63, 64);               // the chunk's total
#pragma unroll
      for (int j = 0; j < MARCH_G; ++j) {
        if (c0 + j >= nchunk) break;
        const int k = ((c0 + j) << 6) + lane;
        const float alpha = al[j];
        const float T = carry * ex[j];
        carry *= p[j];
        const float w = alpha * T;                                                    // :31
        if (pass == 0) {
          a_acc += w;
          a_d += (k < S) ? w * (zlds ? s_z[k] : z[k]) : 0.0f;
          a_k += w * (float)k;
        }
        if (emit) {
          if (w_all && k < S) w_all[(size_t)oray * S + k] = w;
          const bool sh = (k < S) && (w > f.weight_thres);                            // :622
          const unsigned long long m = __ballot(sh);
          if (sh) {
            const int pos = nsh + __popcll(m & ((1ull << lane) - 1ull));
            cidx[(size_t)ray * S + pos] = (uint16_t)k;
            cw[(size_t)ray * S + pos] = w;
          }
          nsh += __popcll(m);
        }
      }
    }
    if (pass == 0) {
      acc = wave_sum(a_acc);                                                        // :614
      dsum = wave_sum(a_d);
      kbar = wave_sum(a_k);
    }
  }
  LRF_MTICK(2);
  if (lane == 0) {
    depth[oray] = dsum / dn;                                                        // :615
    acc_ws[ray] = acc;
    ncomp[ray] = nsh;
    if (f.rdir) *reinterpret_cast<float4*>(f.rdir + (size_t)ray * 4) = make_float4(dh[0], dh[1], dh[2], dn);
    if (gsum) {
      // gsum[lb] = the 32-sample tiles of this workgroup's rays (k_shade3 scans these sums instead of every ray's count).
      // One LDS add per wave, no barrier behind the early return above: the wave that finds all the others' adds
      // in front of its own writes the sum (at most 16 rays x 128 tiles: the count of waves sits above bit 20).
      const unsigned tiles = (unsigned)((nsh + MARCH_TILE - 1) / MARCH_TILE);
      const unsigned old = atomicAdd(s_gcomb, (1u << 20) | tiles);
      if ((int)(old >> 20) + 1 == min(nw, R - lb * nw)) gsum[lb] = (int)((old & 0xfffffu) + tiles);
    }
  }
  LRF_MTICK(3);
  if (TIMED && f.dump && lane == 0) {
    unsigned long long* dp = reinterpret_cast<unsigned long long*>(f.dump) + (size_t)ray * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) dp[i] = tk[i];
  }
#undef LRF_MTICK
}

template <bool LDSL, bool MULTI = false>
__global__ __launch_bounds__(1024) void k_march(
    typename FieldArg<MULTI>::type fin, const float* __restrict__ rays, const float* __restrict__ z, int R, int S,
    uint32_t flags, float floater,
    float* __restrict__ depth, float* __restrict__ acc_ws, float* __restrict__ w_all,
    int* __restrict__ ncomp, int* __restrict__ gsum /* [workgroups] tiles of each workgroup's rays; or null */,
    uint16_t* __restrict__ cidx, float* __restrict__ cw,
    float* __restrict__ feat_out /* [R,S] density feature, -inf where not evaluated; or null */, int zlds) {
  march_body<LDSL, MULTI, false>(fin, rays, z, R, S, flags, floater, depth, acc_ws, w_all, ncomp, gsum, cidx, cw, feat_out, zlds != 0);
}
// the same with the phase clocks (fin.dump: [R][4] uint64)
template <bool LDSL>
__global__ __launch_bounds__(1024) void k_march_timed(
    DField fin, const float* __restrict__ rays, const float* __restrict__ z, int R, int S,
    uint32_t flags, float floater,
    float* __restrict__ depth, float* __restrict__ acc_ws, float* __restrict__ w_all,
    int* __restrict__ ncomp, int* __restrict__ gsum, uint16_t* __restrict__ cidx, float* __restrict__ cw,
    float* __restrict__ feat_out, int zlds) {
  march_body<LDSL, false, true>(fin, rays, z, R, S, flags, floater, depth, acc_ws, w_all, ncomp, gsum, cidx, cw, feat_out, zlds != 0);
}

// Exclusive prefix sum of per-ray tile counts: toff[r] = sum_{q<r} ceil(ncomp[q]/16),
// toff[R] = total.  One 1024-thread block; replaces a device-wide atomic work queue (one
// atomic word saturates at ~88 dequeues/us on this chip -- 52K pulls cost 0.59 ms).
__global__ __launch_bounds__(1024) void k_scan_tiles(const int* __restrict__ ncomp, int R, int* __restrict__ toff) {
  __shared__ int s_wave[16];
  __shared__ int s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < R; base += 1024) {
    const int r = base + tid;
    const int v = r < R ? (ncomp[r] + ITEM - 1) / ITEM : 0;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int woff = 0;
    for (int q = 0; q < wave; ++q) woff += s_wave[q];
    const int carry = s_carry;
    if (r < R) toff[r] = carry + woff + incl - v;
    __syncthreads();
    if (tid == 1023) s_carry = carry + woff + incl;
    __syncthreads();
  }
  if (tid == 0) toff[R] = s_carry;
}

// --------------------------------------------------------------------------- shade
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// appearance products for this lane's 6 channels of each plane (tensoRF.py:153-195):
// lane (s, g) of a tile owns channels 6g..6g+5 of plane p -> K-slot g of MFMA k-step (p, j).
// appearance products of lane group g for plane p: eight slots (six channels + two zero pads)
// per tap, read as two aligned float4 of the padded 128-byte texel (tensoRF.py:153-195)
template <int p>
__device__ __forceinline__ void gather_app6_plane(const DField& f, const float u[3], int g, float X[8]) {
  int x0, x1, y0, y1, l0, l1; float tx, ty, tl;
  tap1d(u[MAT0[p]], f.pw[p], x0, x1, tx);
  tap1d(u[MAT1[p]], f.ph[p], y0, y1, ty);
  tap1d(u[VEC[p]],  f.ll[p], l0, l1, tl);
  const float* pl = f.aplane[p] + 8 * g;
  const float* q00 = pl + ((size_t)y0 * f.pw[p] + x0) * LRF_CAS;
  const float* q10 = pl + ((size_t)y0 * f.pw[p] + x1) * LRF_CAS;
  const float* q01 = pl + ((size_t)y1 * f.pw[p] + x0) * LRF_CAS;
  const float* q11 = pl + ((size_t)y1 * f.pw[p] + x1) * LRF_CAS;
  const float* r0 = f.aline[p] + (size_t)l0 * LRF_CAS + 8 * g;
  const float* r1 = f.aline[p] + (size_t)l1 * LRF_CAS + 8 * g;
  const float w00 = (1.0f - tx) * (1.0f - ty), w10 = tx * (1.0f - ty);
  const float w01 = (1.0f - tx) * ty,          w11 = tx * ty;
  const float wl0 = 1.0f - tl, wl1 = tl;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const float4 a = ld4(q00 + 4 * h), b = ld4(q10 + 4 * h), c = ld4(q01 + 4 * h), d = ld4(q11 + 4 * h);
    const float4 e = ld4(r0 + 4 * h), q = ld4(r1 + 4 * h);
    X[4 * h]     = (a.x * w00 + b.x * w10 + c.x * w01 + d.x * w11) * (e.x * wl0 + q.x * wl1);
    X[4 * h + 1] = (a.y * w00 + b.y * w10 + c.y * w01 + d.y * w11) * (e.y * wl0 + q.y * wl1);
    X[4 * h + 2] = (a.z * w00 + b.z * w10 + c.z * w01 + d.z * w11) * (e.z * wl0 + q.z * wl1);
    X[4 * h + 3] = (a.w * w00 + b.w * w10 + c.w * w01 + d.w * w11) * (e.w * wl0 + q.w * wl1);
  }
}
__device__ __forceinline__ void gather_app6(const DField& f, const float u[3], int g, float X[3][6]) {
  float v[8];
  gather_app6_plane<0>(f, u, g, v);
#pragma unroll
  for (int j = 0; j < 6; ++j) X[0][j] = v[j];
  gather_app6_plane<1>(f, u, g, v);
#pragma unroll
  for (int j = 0; j < 6; ++j) X[1][j] = v[j];
  gather_app6_plane<2>(f, u, g, v);
#pragma unroll
  for (int j = 0; j < 6; ++j) X[2][j] = v[j];
}

// Static, contiguous split of the T = toff[R] tiles over all waves of the grid (tiles cost
// the same, so this is balanced to one tile; consecutive tiles of a wave belong to the same
// ray -> L1/L2 locality; no atomics).  TileWalk yields (ray, j0) for tiles [t, t_end).
struct TileWalk {
  int t, t_end, ray, next_off;
};
__device__ __forceinline__ TileWalk tile_walk_begin(const int* __restrict__ toff, int R) {
  TileWalk tw;
  const int T = toff[R];
  const long long waves = (long long)gridDim.x * (blockDim.x >> 6);
  // XCD-aware order: hardware places block b on XCD b % 8 (speed only, never correctness), so the
  // logical block id below gives every XCD one contiguous eighth of the tile list -- rays that are
  // neighbours in the caller's order (pixels of one image, or direction-sorted rays) share an L2.
  const int nb = gridDim.x;
  const int lb = (nb % 8 == 0) ? (int)(blockIdx.x % 8) * (nb / 8) + (int)(blockIdx.x / 8) : (int)blockIdx.x;
  const long long wid = (long long)lb * (blockDim.x >> 6) + (threadIdx.x >> 6);
  tw.t = __builtin_amdgcn_readfirstlane((int)(wid * T / waves));
  tw.t_end = __builtin_amdgcn_readfirstlane((int)((wid + 1) * T / waves));
  // largest ray with toff[ray] <= t
  int lo = 0, hi = R;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (toff[mid] <= tw.t) lo = mid; else hi = mid;
  }
  tw.ray = __builtin_amdgcn_readfirstlane(lo);            // (wave-uniform: kept in scalar registers across the tile loop)
  tw.next_off = __builtin_amdgcn_readfirstlane(toff[lo + 1]);
  return tw;
}
// advance to the ray owning tile tw.t (skips rays without shaded samples)
__device__ __forceinline__ void tile_walk_seek(TileWalk& tw, const int* __restrict__ toff) {
  while (tw.next_off <= tw.t) { ++tw.ray; tw.next_off = __builtin_amdgcn_readfirstlane(toff[tw.ray + 1]); }
}

__global__ __launch_bounds__(1024) void k_shade(
    DField f, const float* __restrict__ rays, const float* __restrict__ z, int S,
    const int* __restrict__ toff, int R,
    const int* __restrict__ ncomp, const uint16_t* __restrict__ cidx, const float* __restrict__ cw,
    float* __restrict__ part, int pmax) {
  __shared__ __attribute__((aligned(16))) float img[IMG_FLOATS];
  {
    const float4* src = reinterpret_cast<const float4*>(f.mlp);
    float4* dst = reinterpret_cast<float4*>(img);
    for (int i = threadIdx.x; i < IMG_FLOATS / 4; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, s = lane & 15, g = lane >> 4;
  TileWalk tw = tile_walk_begin(toff, R);
  for (; tw.t < tw.t_end; ++tw.t) {
    asm volatile("" ::: "memory");     // keep LDS weight reads inside the loop (no LICM -> no spills)
    tile_walk_seek(tw, toff);
    const int ray = __builtin_amdgcn_readfirstlane(tw.ray);
    const int j0 = (tw.t - (tw.next_off - (ncomp[ray] + ITEM - 1) / ITEM)) * ITEM;
    const int cnt = min(ITEM, ncomp[ray] - j0);

    const float* rp = rays + (size_t)ray * 6;
    const float o[3] = {rp[0], rp[1], rp[2]};
    const float dn = sqrtf(rp[3] * rp[3] + rp[4] * rp[4] + rp[5] * rp[5]);
    const float dh[3] = {rp[3] / dn, rp[4] / dn, rp[5] / dn};
    // view-direction part of mlp_view.0 + bias: constant per ray (tensorBase.py:131-132;
    // viewdirs detached :628)
    float vb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float4 wv = *reinterpret_cast<const float4*>(&img[IMG_W3V + 4 * c]);
      vb[c] = wv.w + wv.x * dh[0] + wv.y * dh[1] + wv.z * dh[2];
    }
    {
      const bool valid = s < cnt;
      const size_t ci = (size_t)ray * S + j0 + (valid ? s : 0);
      const int k = cidx[ci];
      const float w = valid ? cw[ci] : 0.0f;
      float x[3], u[3];
      sample_point(f, o, dh, z[k], x, u);
      float X[3][6];
      gather_app6(f, u, g, X);

      // basis: feat = basis_mat.weight @ (plane*line)            (tensoRF.py:196)
      f32x4 fe[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
      for (int p = 0; p < 3; ++p) {
#pragma unroll
        for (int t1 = 0; t1 < 2; ++t1) {
          const float* ap = &img[IMG_BAS + ((t1 * 3 + p) * 64 + lane) * 8];
          const float4 a0 = *reinterpret_cast<const float4*>(ap);
          const float2 a1 = *reinterpret_cast<const float2*>(ap + 4);
          fe[t1] = mfma4(a0.x, X[p][0], fe[t1]);
          fe[t1] = mfma4(a0.y, X[p][1], fe[t1]);
          fe[t1] = mfma4(a0.z, X[p][2], fe[t1]);
          fe[t1] = mfma4(a0.w, X[p][3], fe[t1]);
          fe[t1] = mfma4(a1.x, X[p][4], fe[t1]);
          fe[t1] = mfma4(a1.y, X[p][5], fe[t1]);
        }
      }
      // layer 1: relu(W1 feat + b1)                               (tensorBase.py:129-130)
      f32x4 h1[8];
#pragma unroll
      for (int t1 = 0; t1 < 8; ++t1) h1[t1] = *reinterpret_cast<const f32x4*>(&img[IMG_B1 + 16 * t1 + 4 * g]);
#pragma unroll
      for (int t0 = 0; t0 < 2; ++t0) {
#pragma unroll
        for (int t1 = 0; t1 < 8; ++t1) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(&img[IMG_W1 + ((t1 * 2 + t0) * 64 + lane) * 4]);
#pragma unroll
          for (int r = 0; r < 4; ++r) h1[t1] = mfma4(a[r], fe[t0][r], h1[t1]);
        }
      }
#pragma unroll
      for (int t1 = 0; t1 < 8; ++t1)
#pragma unroll
        for (int r = 0; r < 4; ++r) h1[t1][r] = fmaxf(h1[t1][r], 0.0f);
      // layer 2: relu(W2 h1 + b2)
      f32x4 h2[8];
#pragma unroll
      for (int t1 = 0; t1 < 8; ++t1) h2[t1] = *reinterpret_cast<const f32x4*>(&img[IMG_B2 + 16 * t1 + 4 * g]);
#pragma unroll
      for (int t0 = 0; t0 < 8; ++t0) {
#pragma unroll
        for (int t1 = 0; t1 < 8; ++t1) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(&img[IMG_W2 + ((t1 * 8 + t0) * 64 + lane) * 4]);
#pragma unroll
          for (int r = 0; r < 4; ++r) h2[t1] = mfma4(a[r], h1[t0][r], h2[t1]);
        }
      }
      // head: sigmoid(W3 [h2 ; dhat] + b3) on the VALU            (tensorBase.py:131-133)
      float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
#pragma unroll
      for (int t1 = 0; t1 < 8; ++t1)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float hv = fmaxf(h2[t1][r], 0.0f);
          const float4 wv = *reinterpret_cast<const float4*>(&img[IMG_W3H + (g * 32 + t1 * 4 + r) * 4]);
          o0 += hv * wv.x; o1 += hv * wv.y; o2 += hv * wv.z;
        }
      o0 += __shfl_xor(o0, 16, 64); o1 += __shfl_xor(o1, 16, 64); o2 += __shfl_xor(o2, 16, 64);
      o0 += __shfl_xor(o0, 32, 64); o1 += __shfl_xor(o1, 32, 64); o2 += __shfl_xor(o2, 32, 64);
      float cr = w / (1.0f + expf(-(o0 + vb[0])));                 // :133, :632
      float cg = w / (1.0f + expf(-(o1 + vb[1])));
      float cb = w / (1.0f + expf(-(o2 + vb[2])));
#pragma unroll
      for (int dd = 1; dd < 16; dd <<= 1) {
        cr += __shfl_xor(cr, dd, 64); cg += __shfl_xor(cg, dd, 64); cb += __shfl_xor(cb, dd, 64);
      }
      if (lane == 0) {
        float* pp = part + ((size_t)ray * pmax + j0 / ITEM) * 3;
        pp[0] = cr; pp[1] = cg; pp[2] = cb;
      }
    }
  }
}

// ------------------------------------------------------------------ split-bf16 products, 16-sample tiles
// The training kernels (lrf_backward.inl) run every GEMM of the colour network on v_mfma_f32_16x16x32_bf16 with both
// operands split into hi + lo bf16 (x ~ hi + lo to 2^-16): acc += Al*Bh + Ah*Bl + Ah*Bh, fp32 accumulate -- ~1e-5
// relative error per product, inside the 1e-4 parity budget (tests/test_gpu_parity.py).
// Rounds 1-2 issued these MFMAs by hand (tied accumulators, four wait states behind each, operands held for 48 more)
// because renders differed from run to run and a late operand read was suspected.  It was not that
// (scripts/ubench/mfma_war.hip: the pipe reads its sources at issue; profiles/r08b: the cause was packed fp32 VALU
// arithmetic): the chain is plain builtins now, the three terms term-major over the NT accumulators of a step so that
// consecutive MFMAs never depend on each other.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split8(const float v[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h = (__bf16)v[j];             // v_cvt_pk_bf16_f32, round-to-nearest-even
    hi[j] = h;
    lo[j] = (__bf16)(v[j] - (float)h);
  }
}
template <int NT>
__device__ __forceinline__ void settle(f32x4*) {}          // (was: wait states behind a hand-issued chain)
__device__ __forceinline__ void mfma_bf16_acc(bf16x8 a, bf16x8 b, f32x4& acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ bf16x8 lds_frag(const uint4* img, int frag, int part, int lane) {
  return __builtin_bit_cast(bf16x8, img[(frag * 2 + part) * 64 + lane]);
}
// acc[t1] += A(frag0 + t1*stride) x B for t1 in [0, NT), three-term split product; the accumulators are taken G at a
// time (the training kernels run 1024-thread workgroups: 128 registers per lane, a fragment pair costs eight)
template <int NT, int G = (NT < 2 ? NT : 2)>
__device__ __forceinline__ void gemm_step(const uint4* img, int frag0, int stride, int lane,
                                          bf16x8 bh, bf16x8 bl, f32x4* acc) {
#pragma unroll
  for (int t0 = 0; t0 < NT; t0 += G) {
    bf16x8 ah[G], al[G];
#pragma unroll
    for (int t1 = 0; t1 < G; ++t1)
      if (t0 + t1 < NT) { ah[t1] = lds_frag(img, frag0 + (t0 + t1) * stride, 0, lane); al[t1] = lds_frag(img, frag0 + (t0 + t1) * stride, 1, lane); }
#pragma unroll
    for (int t1 = 0; t1 < G; ++t1) if (t0 + t1 < NT) mfma_bf16_acc(al[t1], bh, acc[t0 + t1]);
#pragma unroll
    for (int t1 = 0; t1 < G; ++t1) if (t0 + t1 < NT) mfma_bf16_acc(ah[t1], bl, acc[t0 + t1]);
#pragma unroll
    for (int t1 = 0; t1 < G; ++t1) if (t0 + t1 < NT) mfma_bf16_acc(ah[t1], bh, acc[t0 + t1]);
  }
}

}  // namespace lrf
#include "lrf_tiles.inl"
#include "lrf_shade3.inl"
namespace lrf {

// (the plain-loop engine of LRF_FLAG_MLP_VALU is k_shade_gen of lrf_generic.inl: the same kernel serves every non-default
// network configuration)

// rgb_map = sum_k w_k rgb_k (+ 1 - acc)                        (tensorBase.py:632-634)
__global__ void k_finalize(int R, int pmax, uint32_t flags, const int* __restrict__ ncomp,
                           const float* __restrict__ acc, const float* __restrict__ part,
                           float* __restrict__ rgb, float* __restrict__ acc_out, const int* __restrict__ perm) {
  const int ray = blockIdx.x * blockDim.x + threadIdx.x;
  if (ray >= R) return;
  const int oray = perm ? perm[ray] : ray;
  const int nit = (ncomp[ray] + ITEM - 1) / ITEM;
  float r = 0.0f, g = 0.0f, b = 0.0f;
  for (int i = 0; i < nit; ++i) {
    const float* pp = part + ((size_t)ray * pmax + i) * 3;
    r += pp[0]; g += pp[1]; b += pp[2];
  }
  if (flags & LRF_FLAG_WHITE_BG) {
    const float bg = 1.0f - acc[ray];
    r += bg; g += bg; b += bg;
  }
  rgb[(size_t)oray * 3 + 0] = r; rgb[(size_t)oray * 3 + 1] = g; rgb[(size_t)oray * 3 + 2] = b;
  if (acc_out) acc_out[oray] = acc[ray];
}

// ---------------------------------------------------------------------------- ray sorting (LRF_FLAG_SORT_RAYS)
// Rays are independent, so the batch may be rendered in any order; the caller's order is usually the worst one (random
// pixels of a few views; random directions in the benchmark): the 256 CUs then gather from everywhere at once and an
// XCD's 4 MB L2 sees the whole 35-160 MB field.  One 1024-thread workgroup sorts the batch by a 15-bit direction key
// (cube face of d / |d|, then the Morton code of the two in-face coordinates at 6 bits each) with a bitonic network on
// (key << 16 | index) words in LDS, writes the sorted copy of the rays and the slot -> ray permutation.  Everything after
// it indexes rays by slot; only what the caller sees (rgb, depth, weights, g_rgb, g_depth, g_rays) goes through `perm`.
// With the XCD-aware block order of the kernels, an XCD then renders one contiguous eighth of the direction sphere.
__device__ __forceinline__ uint32_t ray_dir_key(const float* __restrict__ rp) {
  const float x = rp[3], y = rp[4], z = rp[5];
  const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
  int face; float m, u, v;
  if (ax >= ay && ax >= az) { face = x < 0.0f ? 1 : 0; m = ax; u = y; v = z; }
  else if (ay >= az)        { face = y < 0.0f ? 3 : 2; m = ay; u = x; v = z; }
  else                      { face = z < 0.0f ? 5 : 4; m = az; u = x; v = y; }
  m = fmaxf(m, 1e-30f);
  const int iu = min(63, max(0, (int)((u / m * 0.5f + 0.5f) * 64.0f)));
  const int iv = min(63, max(0, (int)((v / m * 0.5f + 0.5f) * 64.0f)));
  uint32_t mort = 0;
#pragma unroll
  for (int b = 0; b < 6; ++b) mort |= (uint32_t)((iu >> b) & 1) << (2 * b) | (uint32_t)((iv >> b) & 1) << (2 * b + 1);
  return ((uint32_t)face << 12) | mort;
}
__global__ __launch_bounds__(1024) void k_sort_rays(const float* __restrict__ rays, int R, int N /* pow2 >= R */,
                                                    float* __restrict__ rays_s, int* __restrict__ perm) {
  extern __shared__ uint32_t s_key[];
  const int tid = threadIdx.x;
  for (int i = tid; i < N; i += 1024) s_key[i] = i < R ? (ray_dir_key(rays + (size_t)i * 6) << 16) | (uint32_t)i : 0xffffffffu;
  __syncthreads();
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < N / 2; t += 1024) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;        // the pair (lo, lo + j)
        const uint32_t a = s_key[lo], b = s_key[hi];
        const bool up = (lo & k) == 0;
        if ((a > b) == up) { s_key[lo] = b; s_key[hi] = a; }
      }
      __syncthreads();
    }
  for (int i = tid; i < R; i += 1024) {
    const int src = (int)(s_key[i] & 0xffffu);
    perm[i] = src;
    const float2* sp = reinterpret_cast<const float2*>(rays + (size_t)src * 6);
    float2* dp = reinterpret_cast<float2*>(rays_s + (size_t)i * 6);
    dp[0] = sp[0]; dp[1] = sp[1]; dp[2] = sp[2];
  }
}

// ----------------------------------------------------------------- stand-alone pieces
__global__ void k_density_feature(DField f, const float* __restrict__ u, int P, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const float uu[3] = {u[(size_t)i * 3], u[(size_t)i * 3 + 1], u[(size_t)i * 3 + 2]};
  out[i] = density_feature(f, uu);
}

__global__ void k_app_feature(DField f, const float* __restrict__ u, int P, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const float uu[3] = {u[(size_t)i * 3], u[(size_t)i * 3 + 1], u[(size_t)i * 3 + 2]};
  float acc[LRF_APP_DIM];
  for (int a = 0; a < LRF_APP_DIM; ++a) acc[a] = 0.0f;
  for (int p = 0; p < 3; ++p) {
    int x0, x1, y0, y1, l0, l1; float tx, ty, tl;
    tap1d(uu[MAT0[p]], f.pw[p], x0, x1, tx);
    tap1d(uu[MAT1[p]], f.ph[p], y0, y1, ty);
    tap1d(uu[VEC[p]],  f.ll[p], l0, l1, tl);
    const float* pl = f.aplane[p];
    for (int c = 0; c < LRF_CA; ++c) {
      const int pc = app_pc(c);
      const float v = pl[((size_t)y0 * f.pw[p] + x0) * LRF_CAS + pc] * ((1.0f - tx) * (1.0f - ty))
                    + pl[((size_t)y0 * f.pw[p] + x1) * LRF_CAS + pc] * (tx * (1.0f - ty))
                    + pl[((size_t)y1 * f.pw[p] + x0) * LRF_CAS + pc] * ((1.0f - tx) * ty)
                    + pl[((size_t)y1 * f.pw[p] + x1) * LRF_CAS + pc] * (tx * ty);
      const float l = f.aline[p][(size_t)l0 * LRF_CAS + pc] * (1.0f - tl) + f.aline[p][(size_t)l1 * LRF_CAS + pc] * tl;
      const float xv = v * l;
      for (int a = 0; a < LRF_APP_DIM; ++a) acc[a] += f.basis[a * 72 + p * LRF_CA + c] * xv;
    }
  }
  for (int a = 0; a < LRF_APP_DIM; ++a) out[(size_t)i * LRF_APP_DIM + a] = acc[a];
}

// tensorBase.py:396-417
// TensorBase.sample_ray_contracted (tensorBase.py:419-443) as a public call: pts[r][k] = contract(o_r + d_r z_k).  (The render
// kernels do this per sample in registers; this entry exists for callers of the reference's method.)
__global__ __launch_bounds__(256) void k_sample_contracted(const float* __restrict__ ro, const float* __restrict__ rd,
                                                           const float* __restrict__ z, int R, int S, float* __restrict__ pts) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)R * S) return;
  const int r = (int)(i / S), k = (int)(i % S);
  const float zk = z[k];
  float x = ro[3 * r] + rd[3 * r] * zk, y = ro[3 * r + 1] + rd[3 * r + 1] * zk, w = ro[3 * r + 2] + rd[3 * r + 2] * zk;
  contract3(x, y, w);
  pts[3 * i] = x; pts[3 * i + 1] = y; pts[3 * i + 2] = w;
}

// The ray-independent sample distances of sample_ray_contracted (tensorBase.py:419-437): z[i] = t_i (+ u1_i / h) + 0.1 and
// z[h + i] = 1 / ((1 - s_i) + s_i / 1000) + 0.1 with s_i = t_i (+ u2_i / h), t_i = i / h -- the reference's sixteen
// elementwise launches per training iteration as one; every operation rounded separately, in the reference's order, with
// IEEE divisions: bit-identical to the reference evaluated on the CPU (what the goldens record).  A reference run on a GPU
// evaluates tensor / python_scalar as tensor * (1 / scalar) (ATen's scalar fast path): the linear half then differs by <= 1 ulp
// for h that is not a power of two, the inverse-depth half by up to ~1e-5 relative at its far end (the reciprocal amplifies an ulp of
// s near 1) -- the reference's own GPU / CPU difference, below the tolerances of the path, but not bit-identical
// (test_z_schedule_kernel_vs_reference_expression measures both).
__global__ __launch_bounds__(256) void k_z_schedule(int h, const float* __restrict__ u1, const float* __restrict__ u2, float* __restrict__ z) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h) return;
  const float fh = (float)h;
  const float t = __fdiv_rn((float)i, fh);
  const float a = u1 ? __fadd_rn(t, __fdiv_rn(u1[i], fh)) : t;
  const float s = u2 ? __fadd_rn(t, __fdiv_rn(u2[i], fh)) : t;
  const float den = __fadd_rn(__fmul_rn(1.0f, __fsub_rn(1.0f, s)), __fmul_rn(1.0f / 1e3f, s));   // 1 / near * (1 - t) + 1 / far * t, near = 1
  z[i] = __fadd_rn(a, 1e-1f);
  z[h + i] = __fadd_rn(__fdiv_rn(1.0f, den), 1e-1f);
}

__global__ void k_sample_ray_aabb(const float* __restrict__ rays, float lo0, float lo1, float lo2,
                                  float hi0, float hi1, float hi2, float step, float near_, float far_,
                                  const float* __restrict__ jitter, int R, int N,
                                  float* __restrict__ pts, float* __restrict__ tt, uint8_t* __restrict__ inside) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)R * N) return;
  const int ray = (int)(i / N), k = (int)(i % N);
  const float* rp = rays + (size_t)ray * 6;
  const float lo[3] = {lo0, lo1, lo2}, hi[3] = {hi0, hi1, hi2};
  float tmin = -INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float v = rp[3 + a] == 0.0f ? 1e-6f : rp[3 + a];
    const float ra = (hi[a] - rp[a]) / v, rb = (lo[a] - rp[a]) / v;
    tmin = fmaxf(tmin, fminf(ra, rb));
  }
  tmin = fminf(fmaxf(tmin, near_), far_);
  float rng = (float)k;
  if (jitter) rng += jitter[ray];
  const float t = tmin + step * rng;
  bool in = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float pv = rp[a] + rp[3 + a] * t;
    pts[i * 3 + a] = pv;
    in = in && !(lo[a] > pv) && !(pv > hi[a]);
  }
  tt[i] = t;
  inside[i] = in ? 1 : 0;
}

// ----------------------------------------------------------------------- host side
static DField make_dfield(const LrfField* f) {
  DField d;
  const Layout L = make_layout(f->grid);
  const float* base = reinterpret_cast<const float*>(f->cache);
  for (int p = 0; p < 3; ++p) {
    d.dplane[p] = base + L.dplane[p]; d.dline[p] = base + L.dline[p];
    d.aplane[p] = base + L.aplane[p]; d.aline[p] = base + L.aline[p];
    d.pw[p] = L.pw[p]; d.ph[p] = L.ph[p]; d.ll[p] = L.ll[p];
  }
  d.mlp = base + L.mlp;
  d.mlpb = reinterpret_cast<const uint4*>(base + L.mlpb);
  for (int p = 0; p < 3; ++p) { d.aplane2[p] = base + L.aplane2[p]; d.aline2[p] = base + L.aline2[p]; }
  d.mlpw = reinterpret_cast<const uint4*>(base + L.mlpw);
  d.mlpwt = reinterpret_cast<const uint4*>(base + L.mlpwt);
  d.alpha_vol = f->alpha_vol;
  d.ax = f->alpha_dim[0]; d.ay = f->alpha_dim[1]; d.az = f->alpha_dim[2];
  for (int a = 0; a < 3; ++a) {
    d.lo[a] = f->aabb[a];
    d.hi[a] = f->aabb[3 + a];
    d.inv[a] = 2.0f / (f->aabb[3 + a] - f->aabb[a]);                      // tensorBase.py:321
    d.m_lo[a] = f->alpha_aabb[a];
    d.m_inv[a] = 1.0f / (f->alpha_aabb[3 + a] - f->alpha_aabb[a]) * 2.0f;  // tensorBase.py:44
  }
  d.density_shift = f->density_shift; d.distance_scale = f->distance_scale; d.weight_thres = f->weight_thres;
  d.term_T = f->term_T > 0.0f ? f->term_T : 0.0f;
  d.dump = nullptr;
  d.rdir = nullptr;
  d.perm = nullptr;
  d.basis = f->basis; d.w1 = f->w1; d.b1 = f->b1; d.w2 = f->w2; d.b2 = f->b2; d.w3 = f->w3; d.b3 = f->b3;
  d.fea_pe = f->fea_pe; d.view_pe = f->view_pe; d.fc = f->feature_c ? f->feature_c : LRF_FEATC;
  return d;
}

}  // namespace lrf

#include "lrf_generic.inl"
#include "lrf_forward.inl"
#include "lrf_backward.inl"
namespace lrf {
// Every kernel that may ask for more than 64 KB of dynamic LDS, with the most it can ask for.  The forward's rows carry the
// budgets its plans are held to (lrf_forward.inl): plan_march keeps a k_march<true> workgroup within MARCH_LDS_BUDGET + the tail
// (static_assert there) and a k_march<false> one within MARCH_LDS_NOLINES; plan_shade3 keeps every form of the colour kernel
// within SHADE3_LDS_CAP.
static hipError_t lds_opt_in() {
  constexpr int L160 = 160 * 1024, MARCH = (int)MARCH_LDS_OPT_IN, MARCH_NL = (int)MARCH_LDS_NOLINES, SHADE3 = (int)SHADE3_LDS_CAP;
  static const struct { const void* k; int bytes; } tab[] = {
    {reinterpret_cast<const void*>(&k_sort_rays), LRF_SORT_MAX_R * 4},
    {reinterpret_cast<const void*>(&k_march<true>), MARCH},
    {reinterpret_cast<const void*>(&k_march<true, true>), MARCH},
    {reinterpret_cast<const void*>(&k_march_timed<true>), MARCH},
    {reinterpret_cast<const void*>(&k_march<false>), MARCH_NL},       // four alpha slices of S = 4096 are 64 KB, + the combine word of gsum
    {reinterpret_cast<const void*>(&k_march_timed<false>), MARCH_NL},
    {reinterpret_cast<const void*>(&k_shade3<8, true, false>), SHADE3},
    {reinterpret_cast<const void*>(&k_shade3<8, false, false>), SHADE3},
    {reinterpret_cast<const void*>(&k_shade3<8, true, true>), SHADE3},
    {reinterpret_cast<const void*>(&k_shade3<8, true, false, true>), SHADE3},
    {reinterpret_cast<const void*>(&k_shade3<8, false, false, true>), SHADE3},
    {reinterpret_cast<const void*>(&k_shade3m<8, false>), SHADE3},
    {reinterpret_cast<const void*>(&k_shade_gen<32, false>), L160 - 1024},
    {reinterpret_cast<const void*>(&k_shade_gen<32, true>), L160 - 1024},
    {reinterpret_cast<const void*>(&k_gen_dgrad<32>), L160 - 1024},
    {reinterpret_cast<const void*>(&k_gen_dgrad<16>), L160 - 1024},
    {reinterpret_cast<const void*>(&k_scatter_plane<LRF_CA, true, LRF_APP_NT, false>), L160},
    {reinterpret_cast<const void*>(&k_scatter_plane<LRF_CA, true, LRF_APP_NT, true>), L160},
    {reinterpret_cast<const void*>(&k_scatter_plane<LRF_CD, false, 512, true>), L160},
    {reinterpret_cast<const void*>(&k_scatter_line<LRF_CA, true, 1024>), L160},
    {reinterpret_cast<const void*>(&k_scatter_line<LRF_CD, false, 1024>), L160},
    {reinterpret_cast<const void*>(&k_bwd_ray), 14 * LRF_MAX_S_TRAIN * 4 + BIN_MAX * 4},
    {reinterpret_cast<const void*>(&k_train_dgrad3<8>), L160 - 256},
    {reinterpret_cast<const void*>(&k_train_app3<8, false>), 128 * 1024},
    {reinterpret_cast<const void*>(&k_train_app3<8, true>), 128 * 1024},
    {reinterpret_cast<const void*>(&k_scatter_fix<LRF_CD, false, FIX_NT>), L160},
    {reinterpret_cast<const void*>(&k_scatter_fix<LRF_CA, true, FIX_NT>), L160},
    {reinterpret_cast<const void*>(&k_scatter_fix<LRF_CA, true, FIX_NT, 4>), L160},
    {reinterpret_cast<const void*>(&k_scatter_det<LRF_CD, false, FIX_NT>), L160},
    {reinterpret_cast<const void*>(&k_scatter_det<LRF_CA, true, FIX_NT>), L160},
    {reinterpret_cast<const void*>(&k_scatter_det<LRF_CA, true, FIX_NT, 4>), L160},
    {reinterpret_cast<const void*>(&k_wgrad_w2w3<128>), (int)w23_lds(128)},
    {reinterpret_cast<const void*>(&k_wgrad_w2w3<64>), (int)w23_lds(64)},
  };
  static std::once_flag once[64];        // per device; a launch on another host thread must not overtake the opt-in
  static hipError_t err[64];
  int dev = 0;
  const hipError_t e0 = hipGetDevice(&dev);
  if (e0 != hipSuccess) return e0;
  std::call_once(once[dev & 63], [dev] {
    hipError_t e = hipSuccess;
    for (const auto& t : tab)
      if (e == hipSuccess) e = hipFuncSetAttribute(t.k, hipFuncAttributeMaxDynamicSharedMemorySize, t.bytes);
    err[dev & 63] = e;
  });
  return err[dev & 63];
}
}  // namespace lrf
#include "lrf_scene.inl"
#include "lrf_adam.inl"
#include "lrf_losses.inl"
#include "lrf_metrics.inl"
#include "lrf_frames.inl"
#include "lrf_select.inl"
#include "lrf_evalgeo.inl"
#include "lrf_encode.inl"
#include "lrf_compact.inl"
#include "lrf_points.inl"
#include "lrf_mesh.inl"
#include "lrf_mesh_clean.inl"
#include "lrf_mesh_simplify.inl"
#include "lrf_mesh_smooth.inl"
#include "lrf_mesh_fill.inl"
#include "lrf_mesh_raster.inl"
#include "lrf_mesh_texture.inl"
#include "lrf_mesh_distance.inl"
#include "lrf_align.inl"
#include "lrf_cloud.inl"
#include "lrf_tsdf_blocks.inl"
#include "lrf_reg.inl"
#include "lrf_mask.inl"
#include "lrf_normals.inl"
#include "lrf_quantile.inl"

namespace lrf {
// Test hook (lrf_debug_block_reduce): the workgroup reductions of lrf_common.h on a caller's rows, one workgroup per row of NT
// floats.  ALL: the every-thread flavour, read out of the LAST thread; else the thread-0 flavour.
template <int NT, bool ALL>
__global__ __launch_bounds__(NT) void k_block_reduce_dbg(const float* __restrict__ in, float* __restrict__ sum32, double* __restrict__ sum64,
                                                         unsigned* __restrict__ bits_min, unsigned* __restrict__ bits_max) {
  __shared__ float red_f[NT / 64];
  __shared__ double red_d[NT / 64];
  __shared__ unsigned red_u[2][NT / 64];
  const float x = in[(size_t)blockIdx.x * NT + threadIdx.x];
  const unsigned u = __float_as_uint(x);
  float s; double d; unsigned lo, hi;
  if (ALL) {
    s = block_sum<NT>(x, red_f);
    d = block_sum<NT>((double)x, red_d);
    lo = block_reduce<NT, true>(u, red_u[0], OpMin());
    hi = block_reduce<NT, true>(u, red_u[1], OpMax());
  } else {
    s = block_sum0<NT>(x, red_f);
    d = block_sum0<NT>((double)x, red_d);
    lo = block_min0<NT>(u, red_u[0]);
    hi = block_max0<NT>(u, red_u[1]);
  }
  if (threadIdx.x == (ALL ? NT - 1 : 0)) {
    sum32[blockIdx.x] = s; sum64[blockIdx.x] = d; bits_min[blockIdx.x] = lo; bits_max[blockIdx.x] = hi;
  }
}
template <int NT>
static int block_reduce_dbg(int B, bool all, hipStream_t st, const float* in, float* sum32, double* sum64, unsigned* lo, unsigned* hi) {
  return all ? launch(k_block_reduce_dbg<NT, true>, B, NT, st, in, sum32, sum64, lo, hi)
             : launch(k_block_reduce_dbg<NT, false>, B, NT, st, in, sum32, sum64, lo, hi);
}
}  // namespace lrf

using namespace lrf;

extern "C" {

int lrf_abi_version(void) { return LRF_ABI_VERSION; }
void lrf_debug_set_dump(float* buf) { g_dump = buf; }
void lrf_debug_march_phases(uint64_t* buf) { g_march_dump = reinterpret_cast<unsigned long long*>(buf); }
void lrf_debug_set_bwd_overlap(int on) { g_bwd_overlap = (on & 1) ? 1 : 0; if (on > 1) g_wgrad_split = (on >> 1) - 1; }   // on = 1 + 2 * (n + 1): k_wgrad_w2w3 on the caller's stream (n > 0) or on the side stream (n = 0)
void lrf_debug_set_lds_lines(int on) { g_no_lds_lines = on ? 0 : 1; }
void lrf_debug_set_pipe_chunk(int rays) { g_pipe_chunk = rays > 0 ? rays : 0; }
void lrf_debug_set_march_rays(int rays) { g_march_rays = (rays == 4 || rays == 8 || rays == 16) ? rays : 0; }
void lrf_debug_set_lds_toff(int on) { g_no_lds_toff = on ? 0 : 1; }
int lrf_debug_tile_ranges(const int32_t* ncomp, int32_t R, int32_t G, int32_t nb, int32_t* gsum, int32_t* ranges,
                          int32_t* toff_out, int32_t* nc_out, void* stream) {
  const char* who = "lrf_debug_tile_ranges";
  if (!ncomp || !gsum || !ranges || !toff_out || !nc_out) return refuse(who, "null argument");
  if (R <= 0 || nb <= 0 || (G != 4 && G != 8 && G != 16)) return refuse(who, "need R > 0, nb > 0 and G in {4, 8, 16}");
  const size_t lds = shade3_toff_lds(R);
  if (lds > 64 * 1024) return refuse(who, "R too large for 64 KB of LDS");
  const unsigned NG = blocks_for(R, G);
  if (NG > SHADE3_MAX_GROUPS) return refuse(who, "more groups than one workgroup scans");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_group_tiles, blocks_for(NG, 256), 256, st, ncomp, R, G, gsum));
  return launch_lds(k_tile_ranges_dbg, nb, 512, lds, st, gsum, ncomp, R, G, reinterpret_cast<int4*>(ranges), toff_out, nc_out);
}
int lrf_debug_tile_reduce(const float* in, int32_t T, float* join, float* sum, void* stream) {
  const char* who = "lrf_debug_tile_reduce";
  if (!in || !join || !sum) return refuse(who, "null argument");
  if (T <= 0) return refuse(who, "need T > 0");
  return launch(k_tile_reduce_dbg, T, 64, reinterpret_cast<hipStream_t>(stream), in, join, sum);
}
int lrf_debug_block_reduce(const float* in, int32_t B, int32_t NT, int32_t every_thread, float* sum32, double* sum64,
                           uint32_t* bits_min, uint32_t* bits_max, void* stream) {
  const char* who = "lrf_debug_block_reduce";
  if (!in || !sum32 || !sum64 || !bits_min || !bits_max) return refuse(who, "null argument");
  if (B <= 0) return refuse(who, "need B > 0");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool all = every_thread != 0;
  if (NT == 64) return block_reduce_dbg<64>(B, all, st, in, sum32, sum64, bits_min, bits_max);
  if (NT == 256) return block_reduce_dbg<256>(B, all, st, in, sum32, sum64, bits_min, bits_max);
  if (NT == 1024) return block_reduce_dbg<1024>(B, all, st, in, sum32, sum64, bits_min, bits_max);
  return refuse(who, "NT is 64, 256 or 1024");
}
#ifdef LRF_SCATTER_PROF
int lrf_debug_scatter_prof(unsigned long long* host_out /* [2][2048][12] */) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(lrf::g_scat_prof), sizeof(unsigned long long) * 2 * 2048 * 12);
}
#endif
void lrf_debug_set_scene_fuse(int on) { g_no_scene_fuse = on ? 0 : 1; }
// Where column `col` of saved row `row` lives, in floats from the start of the ACT (buffer 0) / GRD (buffer 1) region
// of a training workspace (lrf_workspace_layout_bwd gives the regions): the fragment order of lrf_common.h, host side.
// -1 for bad arguments.
int64_t lrf_debug_saved_row_offset(int buffer, uint64_t row, int col) {
  using namespace lrf;
  if (buffer == 0) return (col < 0 || col >= ACT_LD) ? -1 : (int64_t)frag_off((size_t)row, col, ACT_LD);
  if (buffer == 1) {
    if (col < 0 || col >= GRD_LD) return -1;
    if (col >= GRD_DX) return (int64_t)((row >> 4) * (uint64_t)(16 * GRD_LD) + GRD_DX * 16 + (row & 15) * (GRD_LD - GRD_DX) + (col - GRD_DX));   // (the row-major order of the dX block; the other one: lrf_common.h)
    return (int64_t)frag_off((size_t)row, col, GRD_LD);
  }
  if (buffer == 3) {                       // the dX block in its groups order (grd_dx8): col = 24 p + c
    if (col < 0 || col >= 3 * LRF_CA) return -1;
    const int p = col / LRF_CA, c = col % LRF_CA;
    return (int64_t)((row >> 4) * (uint64_t)(16 * GRD_LD) + GRD_DX * 16 + (((p * 3 + (c >> 3)) * 16 + (int)(row & 15)) << 3) + (c & 7));
  }
  return -1;
}
const char* lrf_last_error(void) { return lrf_error_slot(); }
char* lrf_error_slot(void) { return g_err; }

size_t lrf_cache_bytes(const int32_t grid[3]) { return make_layout(grid).total * sizeof(float); }

int lrf_pack_field(const LrfParams* p, void* cache, void* stream) {
  if (!p || !cache) return refuse("lrf_pack_field", "null argument");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const Layout L = make_layout(p->grid);
  float* base = reinterpret_cast<float*>(cache);
  PackTab tab;
  int wmax = 1, hmax = 1;
  for (int q = 0; q < 3; ++q) {
    tab.s[4 * q + 0] = PackSeg{p->density_plane[q], base + L.dplane[q], LRF_CD, L.ph[q], L.pw[q], LRF_CD, 0};
    tab.s[4 * q + 1] = PackSeg{p->app_plane[q], base + L.aplane[q], LRF_CA, L.ph[q], L.pw[q], LRF_CAS, 1};
    tab.s[4 * q + 2] = PackSeg{p->density_line[q], base + L.dline[q], LRF_CD, 1, L.ll[q], LRF_CD, 0};
    tab.s[4 * q + 3] = PackSeg{p->app_line[q], base + L.aline[q], LRF_CA, 1, L.ll[q], LRF_CAS, 1};
    tab.s[12 + 2 * q + 0] = PackSeg{p->app_plane[q], base + L.aplane2[q], LRF_CA, L.ph[q], L.pw[q], LRF_CA, 0};
    tab.s[12 + 2 * q + 1] = PackSeg{p->app_line[q], base + L.aline2[q], LRF_CA, 1, L.ll[q], LRF_CA, 0};
    wmax = max(wmax, max(L.pw[q], L.ll[q]));
    hmax = max(hmax, L.ph[q]);
  }
  static_assert(IMG_FLOATS <= 26880 && IMGB_ALL * 4 <= 26880 && W32_ALL_U4 * 4 <= 26880 && W32T_ALL_U4 * 4 <= 26880, "slice 18 of k_pack_planes covers every network image");
  PackMlp pm;
  pm.mlp = base + L.mlp; pm.mlpb = reinterpret_cast<uint32_t*>(base + L.mlpb); pm.mlpw = reinterpret_cast<uint32_t*>(base + L.mlpw);
  pm.mlpwt = reinterpret_cast<uint32_t*>(base + L.mlpwt);
  pm.mode = gen_is_default(p->fea_pe, p->view_pe, p->feature_c ? p->feature_c : LRF_FEATC) ? 0 : 1;   // the generic engine reads the parameter tensors themselves
  return launch(k_pack_planes, dim3(blocks_for(wmax, 128), hmax, 19), 128, st, tab, *p, pm, 0);
}

int lrf_density_feature(const LrfField* f, const float* u, int32_t P, float* out, void* stream) {
  if (!f || !f->cache || !u || !out) return refuse("lrf_density_feature", "null argument");
  if (P <= 0) return 0;
  return launch(k_density_feature, blocks_for(P, 256), 256, reinterpret_cast<hipStream_t>(stream), make_dfield(f), u, P, out);
}

int lrf_app_feature(const LrfField* f, const float* u, int32_t P, float* out, void* stream) {
  if (!f || !f->cache || !u || !out || !f->basis) return refuse("lrf_app_feature", "null argument");
  if (P <= 0) return 0;
  return launch(k_app_feature, blocks_for(P, 128), 128, reinterpret_cast<hipStream_t>(stream), make_dfield(f), u, P, out);
}

int lrf_sample_ray_aabb(const float* rays, const float aabb[6], float step_size, float near_, float far_,
                        const float* jitter, int32_t R, int32_t N, float* pts, float* t, uint8_t* inside,
                        void* stream) {
  if (!rays || !aabb || !pts || !t || !inside) return refuse("lrf_sample_ray_aabb", "null argument");
  const size_t n = (size_t)R * N;
  if (!n) return 0;
  return launch(k_sample_ray_aabb, (unsigned)((n + 255) / 256), 256, reinterpret_cast<hipStream_t>(stream),
                rays, aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5], step_size, near_, far_, jitter, R, N, pts, t, inside);
}

int lrf_z_schedule(int32_t h, const float* u1, const float* u2, float* z, void* stream) {
  const char* who = "lrf_z_schedule";
  if (h <= 0 || !z) return refuse(who, "need h > 0 and an output of 2 h floats");
  if ((u1 == nullptr) != (u2 == nullptr)) return refuse(who, "both jitters or none");
  return launch(k_z_schedule, blocks_for(h, 256), 256, reinterpret_cast<hipStream_t>(stream), h, u1, u2, z);
}

int lrf_sample_ray_contracted(const float* rays_o, const float* rays_d, const float* z, int32_t R, int32_t S,
                              float* pts, void* stream) {
  if (!rays_o || !rays_d || !z || !pts) return refuse("lrf_sample_ray_contracted", "null argument");
  const size_t n = (size_t)R * S;
  if (!n) return 0;
  return launch(k_sample_contracted, (unsigned)((n + 255) / 256), 256, reinterpret_cast<hipStream_t>(stream), rays_o, rays_d, z, R, S, pts);
}

}  // extern "C"
