// lrf_shade3.inl -- the colour stage on v_mfma_f32_32x32x16_bf16, 32 samples per wave (default engine since round 3).
//
// What k_shade2 (16 samples per wave on v_mfma_f32_16x16x32_bf16) taught (profiles/r07c_round_end.md): every 16-sample
// tile re-reads the 92 KB weight image from LDS, the three-term products ran as dependent MFMA triples with hand-placed
// wait states, and 16 waves per CU drifted into lockstep (all gathering, then all multiplying).  This kernel:
//   * 32 samples per wave: lane (n = lane & 31, h = lane >> 5) = (sample, K half).  One A fragment now feeds 32 columns:
//     half the LDS fragment traffic per sample, and the D registers of a layer are again the B operand of the next
//     (K permutation folded into the packed weights, lrf_common.h W32_*): no LDS round trip, no lane movement.
//   * compiler-scheduled builtins.  scripts/ubench/mfma_war.hip (profiles/r08a) shows the matrix pipe reads its sources at
//     issue: hipcc's hazard table is sufficient, the hand-issued chain of k_shade2 and its 299 s_nop per tile were not
//     needed.  The three terms of a split product go term-major over independent accumulators, so no MFMA waits for the
//     one issued just before it.
//   * 512-thread workgroups, one per CU: 8 waves, two per SIMD, up to 256 registers each; tiles come from a per-workgroup
//     queue, and each wave fetches the header of its next tile one tile ahead.  (Forcing the two waves of a SIMD into
//     opposite phases with s_barrier -- one gathers while the other multiplies -- was measured: 153 vs 139 us; 12 waves
//     with 168 registers: 156 us, the chain spills.  profiles/r08c.)
//   * dense 24-channel appearance texels (96 B): lane half h reads channels 12 h .. 12 h + 11 of a tap as three aligned
//     float4: 54 wave-level loads per 32 samples (k_shade2: 72), five basis K-steps of 16 instead of six.
//   * a workgroup owns WHOLE rays (its tile range is cut at ray boundaries): every ray's tile partials are summed, in
//     tile order, by the workgroup that wrote them -- no hand-off between workgroups, no counter, no cross-XCD visibility
//     protocol (the boundary rays of k_shade2<FUSE> needed one).
// Arithmetic per sample as k_shade2: split-bf16 three-term products, fp32 accumulate, VALU head, hardware exp2 / rcp.
#pragma once

namespace lrf {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int ITEM3 = 32;          // compact samples per work item of k_shade3 = one 32-column MFMA tile

__device__ __forceinline__ bf16x8 w32_frag(const uint4* img, int frag, int part, int lane) {
  return __builtin_bit_cast(bf16x8, img[(frag * 2 + part) * 64 + lane]);
}
// hi = bf16(v) (round to nearest even), lo = bf16(v - hi), two values at a time: one packed conversion gives both hi
// halves, a shift and a mask turn them back into floats, a packed subtract forms both remainders (2.5 VALU instructions per
// value; the element-wise form costs 4)
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split8c(const float v[8], bf16x8& hi, bf16x8& lo) {
  uint32_t H[4], L[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2v ab = {v[2 * j], v[2 * j + 1]};
    const uint32_t p = __builtin_bit_cast(uint32_t, __builtin_convertvector(ab, bf16x2v));
    const f32x2v hv = {__uint_as_float(p << 16), __uint_as_float(p & 0xffff0000u)};
    const f32x2v r = ab - hv;                                  // one packed subtract (straight halves: finding 17 does not apply): k_shade3 119.2 -> 116.8 us
    H[j] = p;
    L[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(r, bf16x2v));
  }
  hi = __builtin_bit_cast(bf16x8, make_uint4(H[0], H[1], H[2], H[3]));
  lo = __builtin_bit_cast(bf16x8, make_uint4(L[0], L[1], L[2], L[3]));
}
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// acc[m] += A(frag0 + m * stride) x B for NM output tiles, three-term split product, term-major: the MFMAs that follow
// each other write different accumulators
template <int NM>
__device__ __forceinline__ void mma3_step(const uint4* img, int frag0, int stride, int lane, bf16x8 bh, bf16x8 bl, f32x16* acc) {
  bf16x8 ah[NM], al[NM];
#pragma unroll
  for (int m = 0; m < NM; ++m) { ah[m] = w32_frag(img, frag0 + m * stride, 0, lane); al[m] = w32_frag(img, frag0 + m * stride, 1, lane); }
#pragma unroll
  for (int m = 0; m < NM; ++m) acc[m] = mfma32(al[m], bh, acc[m]);
#pragma unroll
  for (int m = 0; m < NM; ++m) acc[m] = mfma32(ah[m], bl, acc[m]);
#pragma unroll
  for (int m = 0; m < NM; ++m) acc[m] = mfma32(ah[m], bh, acc[m]);
}

// The tail's lane sums without LDS round trips (ds_bpermute_b32 shares the LDS pipe with the SIMD partner's fragment reads).
// Both give, in every lane and bit for bit, what the __shfl_xor butterflies gave (fp32 addition commutes; no NaNs):
//   join_halves32(v) = v + __shfl_xor(v, 32): v_permlane32_swap of v with itself leaves the low half twice in one
//     register and the high half twice in the other.
//   half_sum32(v) = the ladder v += __shfl_xor(v, d), d = 1, 2, 4, 8, 16, every level with the lane's true xor partner:
//     quad_perm [1,0,3,2] and [2,3,0,1]; lane + 4 for banks 0 and 2 of a row and lane - 4 for banks 1 and 3 (two moves under
//     bank masks); row_ror:8; v_permlane16_swap pairs the two rows of a half.  Mirrors (row_half_mirror, row_mirror) would
//     save the second move of the xor 4 level, but they equal the xor partner only while all lanes of a group hold the same
//     value, and in the tile loop they do not: the compiler contracts the first level of half_sum32(w * s) into
//     fma(w, s, partner's rounded product), so the two lanes of a pair differ in the last bit and lane 0's sum is the tree
//     over its true partners.
// All 64 lanes must be enabled (finding 20: a DPP read from a disabled lane returns 0): the tile loop is wave-uniform.
template <int CTRL, int BANKS = 0xf>
__device__ __forceinline__ float dpp_mov(float old, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, 0xf, BANKS, BANKS == 0xf));
}
__device__ __forceinline__ float join_halves32(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float half_sum32(float v) {
  v += dpp_mov<0xB1>(0.0f, v);                                 // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(0.0f, v);                                 // quad_perm [2,3,0,1]
  v += dpp_mov<0x114, 0xa>(dpp_mov<0x104, 0x5>(0.0f, v), v);   // row_shl:4 into banks 0, 2; row_shr:4 into banks 1, 3
  v += dpp_mov<0x128>(0.0f, v);                                // row_ror:8
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// the 12 appearance products of lane half h for plane p: channels 12 h .. 12 h + 11 of the dense texel, three aligned
// float4 per tap (tensoRF.py:153-195); same per-channel arithmetic, in the same order, as gather_app6_plane32
// the 12 appearance products of lane half h for plane p: channels 12 h .. 12 h + 11 of the dense texel, three aligned
// float4 per tap (tensoRF.py:153-195); same per-channel arithmetic, in the same order, as gather_app6_plane32
template <int p>
__device__ __forceinline__ void gather_app12(const DField& f, const AxisTaps& at, int h, float X[12]) {
  const int x0 = at.i0[MAT0[p]], x1 = at.i1[MAT0[p]], y0 = at.i0[MAT1[p]], y1 = at.i1[MAT1[p]];
  const int l0 = at.i0[VEC[p]], l1 = at.i1[VEC[p]];
  const float tx = at.t[MAT0[p]], ty = at.t[MAT1[p]], tl = at.t[VEC[p]];
  const unsigned hb = 48u * (unsigned)h;
  const unsigned row0 = (unsigned)y0 * (unsigned)f.pw[p], row1 = (unsigned)y1 * (unsigned)f.pw[p];
  const unsigned o00 = (row0 + x0) * (LRF_CA * 4u) + hb, o10 = (row0 + x1) * (LRF_CA * 4u) + hb;
  const unsigned o01 = (row1 + x0) * (LRF_CA * 4u) + hb, o11 = (row1 + x1) * (LRF_CA * 4u) + hb;
  const unsigned q0 = (unsigned)l0 * (LRF_CA * 4u) + hb, q1 = (unsigned)l1 * (LRF_CA * 4u) + hb;
  const float w00 = (1.0f - tx) * (1.0f - ty), w10 = tx * (1.0f - ty);
  const float w01 = (1.0f - tx) * ty,          w11 = tx * ty;
  const float wl0 = 1.0f - tl, wl1 = tl;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float4 a = ld4b(f.aplane2[p], o00 + 16 * i), b = ld4b(f.aplane2[p], o10 + 16 * i);
    const float4 c = ld4b(f.aplane2[p], o01 + 16 * i), d = ld4b(f.aplane2[p], o11 + 16 * i);
    const float4 e = ld4b(f.aline2[p], q0 + 16 * i), q = ld4b(f.aline2[p], q1 + 16 * i);
    X[4 * i]     = (a.x * w00 + b.x * w10 + c.x * w01 + d.x * w11) * (e.x * wl0 + q.x * wl1);
    X[4 * i + 1] = (a.y * w00 + b.y * w10 + c.y * w01 + d.y * w11) * (e.y * wl0 + q.y * wl1);
    X[4 * i + 2] = (a.z * w00 + b.z * w10 + c.z * w01 + d.z * w11) * (e.z * wl0 + q.z * wl1);
    X[4 * i + 3] = (a.w * w00 + b.w * w10 + c.w * w01 + d.w * w11) * (e.w * wl0 + q.w * wl1);
  }
}

// per-ray tile counts -> exclusive prefix sum, one 1024-thread block (the caller's R does not fit the LDS copy)
template <int ITEMSZ>
__global__ __launch_bounds__(1024) void k_scan_tiles_n(const int* __restrict__ ncomp, int R, int* __restrict__ toff) {
  __shared__ int s_wave[16];
  __shared__ int s_carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < R; base += 1024) {
    const int r = base + tid;
    const int v = r < R ? (ncomp[r] + ITEMSZ - 1) / ITEMSZ : 0;
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

// first index r in [0, n] with toff[r] >= v (toff non-decreasing, n + 1 entries)
template <class P>
__device__ __forceinline__ int toff_lower_bound_p(P toff, int n, int v) {
  int lo = 0, hi = n + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (toff[mid] >= v) hi = mid; else lo = mid + 1;
  }
  return lo < n ? lo : n;
}

// A colour workgroup's rays [ra, rb) and tiles [T0, T1) of the even split of the tile list (cut at ray boundaries), from
// k_march's group sums instead of a scan over every ray: gsum[g] = tiles of rays [g G, (g + 1) G) (G = 4, 8 or 16, a power of
// two), so toff[g G] is the exclusive scan of gsum -- ceil(R / G) values instead of R.  Every workgroup
//   1. scans the group sums into s_toff[g G] (absolute ray index, as the tile loop reads it) and s_toff[R] = T,
//   2. finds the groups its two cut points fall into (lower bound at group granularity: a count over the registers of step 1),
//   3. loads ncomp for the rays of those groups and the groups between them only, and fills s_toff / s_nc there,
//   4. finishes the two lower bounds inside their groups.
// ra, rb, T0, T1 and every s_toff[r], r in [ra, rb], and s_nc[r], r in [ra, rb), are the integers of the full scan with
// toff_lower_bound_p(toff, R, v) (rb = R for the last workgroup); entries outside [win0, win1] hold nothing.
// Two calls, by all NT threads, with a workgroup barrier between them that the caller places: tile_range_fill (steps 1 - 3; its
// LDS stores are not yet visible), whatever else the caller wants in front of that barrier, __syncthreads(),
// tile_range_finish (step 4).  s_wave: NT / 64 + 2 ints.
typedef __attribute__((address_space(3))) unsigned short lds_u16;
constexpr int TILE_GPT = 8;                                    // group sums per thread: 512 threads hold those of 16384 rays at 4 per group
struct TileRange { int ra, rb, T0, T1, win0, win1; int ga, gb, v0, v1; };   // ga .. v1: from tile_range_fill to tile_range_finish
// step 1's loads on their own: k_shade3 requests them in front of its weight image, whose loads are answered first otherwise
struct GroupSums { int v[TILE_GPT]; };
__device__ __forceinline__ GroupSums tile_group_sums(const int* __restrict__ gsum, int R, int G) {
  const int NG = (R + G - 1) / G, g0 = threadIdx.x * TILE_GPT;
  GroupSums s;
#pragma unroll
  for (int i = 0; i < TILE_GPT; ++i) s.v[i] = g0 + i < NG ? gsum[g0 + i] : 0;
  return s;
}
template <int NT>
__device__ __forceinline__ TileRange tile_range_fill(const GroupSums& gs, const int* __restrict__ ncomp, int R, int G,
                                                     int lb, int nb, lds_int* s_toff, lds_u16* s_nc, int* s_wave) {
  constexpr int NWV = NT / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int NG = (R + G - 1) / G;                              // at most NT * TILE_GPT (the caller's check)
  const int g0 = tid * TILE_GPT;
  int v[TILE_GPT];
#pragma unroll
  for (int i = 0; i < TILE_GPT; ++i) v[i] = gs.v[i];
  if (tid < 2) s_wave[NWV + tid] = 0;                          // the two group counts of step 2
#pragma unroll
  for (int i = 1; i < TILE_GPT; ++i) v[i] += v[i - 1];
  int incl = v[TILE_GPT - 1];
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  int woff = 0, T = 0;
#pragma unroll
  for (int q = 0; q < NWV; ++q) { const int x = s_wave[q]; woff += q < wave ? x : 0; T += x; }
  const int excl = woff + incl - v[TILE_GPT - 1];
  const int v0 = (int)((long long)lb * T / nb), v1 = (int)((long long)(lb + 1) * T / nb);
  const bool last = lb == nb - 1;
  // The first group g in [0, NG] whose first ray's offset (the total, for g = NG) is >= v is the number of groups whose
  // offset is below v (the offsets do not decrease): every thread counts its own, from registers.
  int c0 = 0, c1 = 0;
#pragma unroll
  for (int i = 0; i < TILE_GPT; ++i) {
    const int o = excl + (i ? v[i - 1] : 0);
    const bool in = g0 + i < NG;
    if (in) s_toff[(g0 + i) * G] = o;
    c0 += __popcll(__ballot(in && o < v0));
    c1 += __popcll(__ballot(in && o < v1));
  }
  if (lane == 0 && c0) atomicAdd(&s_wave[NWV], c0);
  if (lane == 0 && c1) atomicAdd(&s_wave[NWV + 1], c1);
  if (tid == 0) s_toff[R] = T;
  __syncthreads();
  const int ga = __builtin_amdgcn_readfirstlane(s_wave[NWV]);
  const int gb = last ? NG : __builtin_amdgcn_readfirstlane(s_wave[NWV + 1]);
  // the cut for v lies in ((g - 1) G, g G]: groups ga - 1 .. gb (one more than rb needs: the tile loop looks at toff[ra + 1])
  TileRange tr;
  tr.win0 = max(ga - 1, 0) * G;
  tr.win1 = min((gb + 1) * G, R);
  for (int r0 = tr.win0; r0 < tr.win1; r0 += NT) {             // (win0 and NT are multiples of G: lane & (G - 1) is the ray's place in its group)
    const int r = r0 + tid, k = lane & (G - 1);
    const int nc = r < tr.win1 ? ncomp[r] : 0;
    const int t = (nc + ITEM3 - 1) / ITEM3;
    int incl = t;
    for (int d = 1; d < G; d <<= 1) {
      const int x = __shfl_up(incl, d, 64);
      if (k >= d) incl += x;
    }
    if (r < tr.win1) {
      s_nc[r] = (unsigned short)nc;
      if (k) s_toff[r] = s_toff[r - k] + incl - t;
    }
  }
  tr.ga = ga; tr.gb = gb; tr.v0 = v0; tr.v1 = v1;
  return tr;
}
__device__ __forceinline__ void tile_range_finish(TileRange& tr, int R, int G, int lb, int nb, lds_int* s_toff) {
  const bool last = lb == nb - 1;
  const int ga = tr.ga, gb = tr.gb, v0 = tr.v0, v1 = tr.v1;
  auto ray_lb = [&](int g, int v) {                            // toff_lower_bound_p's answer, searched inside group g - 1
    if (g == 0) return 0;
    int lo = (g - 1) * G + 1, hi = min(g * G, R);
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_toff[mid] >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
  };
  tr.ra = __builtin_amdgcn_readfirstlane(ray_lb(ga, v0));
  tr.rb = __builtin_amdgcn_readfirstlane(last ? R : ray_lb(gb, v1));
  tr.T0 = __builtin_amdgcn_readfirstlane(s_toff[tr.ra]);
  tr.T1 = __builtin_amdgcn_readfirstlane(s_toff[tr.rb]);
}

// Test hook (lrf_debug_tile_ranges): tile_range_fill / tile_range_finish in a kernel of its own, with group sums that k_group_tiles forms from
// the counts.  Workgroup b (its blockIdx is its place lb in the split: no XCD order here) leaves ranges[b] = {ra, rb, T0,
// T1}, its offsets toff_out[b][ra .. rb] and counts nc_out[b][ra .. rb - 1]; everything else keeps the caller's fill.
__global__ void k_group_tiles(const int* __restrict__ ncomp, int R, int G, int* __restrict__ gsum) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g * G >= R) return;
  int t = 0;
  for (int r = g * G; r < min(g * G + G, R); ++r) t += (ncomp[r] + ITEM3 - 1) / ITEM3;
  gsum[g] = t;
}
__global__ __launch_bounds__(512) void k_tile_ranges_dbg(const int* __restrict__ gsum, const int* __restrict__ ncomp, int R, int G,
                                                         int4* __restrict__ ranges, int* __restrict__ toff_out, int* __restrict__ nc_out) {
  extern __shared__ uint4 s_dyn[];
  __shared__ int s_wave[8 + 2];
  lds_int* s_toff = (lds_int*)s_dyn;
  lds_u16* s_nc = (lds_u16*)(s_toff + R + 1);
  const int lb = blockIdx.x, tid = threadIdx.x;
  TileRange tr = tile_range_fill<512>(tile_group_sums(gsum, R, G), ncomp, R, G, lb, (int)gridDim.x, s_toff, s_nc, s_wave);
  __syncthreads();
  tile_range_finish(tr, R, G, lb, (int)gridDim.x, s_toff);
  if (tid == 0) ranges[lb] = make_int4(tr.ra, tr.rb, tr.T0, tr.T1);
  for (int r = tr.ra + tid; r <= tr.rb; r += 512) {
    toff_out[(size_t)lb * (R + 1) + r] = s_toff[r];
    if (r < tr.rb) nc_out[(size_t)lb * R + r] = s_nc[r];
  }
}

// Test hook (lrf_debug_tile_reduce): the tail's two lane sums on a caller's rows, one wave per row of 64 floats; every lane's result.
__global__ __launch_bounds__(64) void k_tile_reduce_dbg(const float* __restrict__ in, float* __restrict__ join, float* __restrict__ sum) {
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  const float v = in[i];
  join[i] = join_halves32(v);
  sum[i] = half_sum32(v);
}

// What one wave needs to know about a tile before it can gather.  Its vector loads (sample index, weight, direction) are
// issued one tile ahead and first used at the top of the next tile, so the chain sample index -> distance is off the
// critical path; the walk tile -> ray (LDS) and the origin (scalar loads) are waited for where they are issued.
struct Hdr3 {
  int ray, tile_in_ray;          // ray, tile number inside the ray
  uint32_t k2, ksh;              // this lane's sample index into z: bits ksh .. ksh + 15 (ksh = 0 or 16) of the dword k2
  int cnt;                       // samples in the tile (SAVE)
  float wgt;                     // this lane's compositing weight (0 for lanes beyond the tile's count and for K half 1)
  float o[3], d[3];              // ray origin, unit direction
};

// What the training forward keeps for the backward (SAVE; lrf_backward.inl, lrf_common.h): a 32-sample tile t of this kernel
// is the pair 2 t, 2 t + 1 of the backward's 16-row tiles (lane n -> row n & 15 of tile 2 t + (n >> 4)), so a ray owns
// 2 ceil(n / 32) of them and the second of a pair may be empty.
struct SaveOut3 {
  float* crgb;            // [ray * S + j][3] sigmoid colour of compact sample j
  float* act;             // feat rows, 16-row fragment order (ACT_LD)
  uint32_t* relu_bits;    // [16-row tile][layer][lane s + 16 g]: bit 4 t1 + r = unit 16 t1 + 4 g + r is active
  int4* tileinfo;         // [16-row tile] (ray, first compact sample, count, tile number inside the ray)
  int* toff16;            // [R + 1] offsets of the rays' 16-row tiles (= 2 x this kernel's tile offsets)
};

#define LRF_SHADE3_NAME k_shade3
#define LRF_SHADE3_MULTI 0
#include "lrf_shade3_kernel.inl"
#undef LRF_SHADE3_NAME
#undef LRF_SHADE3_MULTI
#define LRF_SHADE3_NAME k_shade3m
#define LRF_SHADE3_MULTI 1
#include "lrf_shade3_kernel.inl"
#undef LRF_SHADE3_NAME
#undef LRF_SHADE3_MULTI

}  // namespace lrf
