/* lrf_debug.h -- test hooks of liblrf_hip.so.  NOT part of the drop-in ABI (include/lrf.h): these are process-wide
 * switches for the diagnostics in scripts/gpu_diag.py and for a few tests; a host thread that flips one while another
 * renders changes that render too.  Production callers never include this header. */
#ifndef LRF_DEBUG_H_
#define LRF_DEBUG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* When set (device buffer of n_CUs * 8 waves * 10 uint64), lrf_render_fwd runs k_shade3<TIMED> and leaves per-wave
 * s_memtime totals there: {prologue, position + taps, gather + split, image requested, tile offsets, chain + head, tiles,
 * finalize, tail (joins, sigmoid, tile sum, store), loop top up to the next header's loads issued}; NULL = off. */
void    lrf_debug_set_dump(float* buf);
/* When set (device buffer of R * 4 uint64, R = the rays of the largest march that follows), every single-field k_march runs
 * with phase clocks and leaves per ray (= per wave) the shader-cycle totals {line and z staging with its barrier, pass A
 * (gathers -> alpha), pass B (scans, weights, compaction), epilogue}; same results as the production kernel.  NULL = off. */
void    lrf_debug_march_phases(uint64_t* buf);
void    lrf_debug_set_lds_lines(int on);          /* k_march: density lines staged in LDS (default on when they fit) */
void    lrf_debug_set_pipe_chunk(int rays);       /* rays per chunk of lrf_render_fwd's two-stream large-batch mode (default 16384; batches of at least two chunks); 0: one pass over the whole batch.  Changes lrf_workspace_bytes: set it before sizing a workspace */
void    lrf_debug_set_march_rays(int rays);       /* k_march: 4, 8 or 16 rays per workgroup where that many fit in LDS with the density lines (else, and with 0: the default choice); k_shade3 reads its group sums at the same size */
void    lrf_debug_set_lds_toff(int on);           /* k_shade3: tile offsets built inside the kernel from k_march's group sums (default on when they fit in LDS); 0 = k_scan_tiles_n first and global offsets, at every batch size */
/* tile_range_fill + tile_range_finish (the prologue of k_shade3) in a kernel of its own: ncomp [R] shaded counts (device), G in {4, 8, 16} rays per
 * group, nb workgroups -> gsum [ceil(R / G)] (scratch), ranges [nb][4] = {ra, rb, T0, T1} of workgroup b, toff_out [nb][R + 1]
 * and nc_out [nb][R]: the offsets of rays ra .. rb and the counts of rays ra .. rb - 1 as workgroup b holds them; other entries
 * are left as the caller filled them.  R up to about 10000 (64 KB of LDS). */
int     lrf_debug_tile_ranges(const int32_t* ncomp, int32_t R, int32_t G, int32_t nb, int32_t* gsum, int32_t* ranges,
                              int32_t* toff_out, int32_t* nc_out, void* stream);
/* k_shade3's tail reductions (csrc/lrf_shade3.inl) on their own: in [T][64] floats (device), one wave per row ->
 * join[t][l] = join_halves32 (in[t][l] + in[t][l ^ 32]) and sum[t][l] = half_sum32 (the sum of the 32-lane half of lane l, in
 * the butterfly's order), every lane's value. */
int     lrf_debug_tile_reduce(const float* in, int32_t T, float* join, float* sum, void* stream);
/* The workgroup reductions every kernel outside the render hot path shares (csrc/lrf_common.h: block_sum, block_sum0, block_min0,
 * block_max0) on their own: in [B][NT] floats (device), NT in {64, 256, 1024}, one workgroup per row -> sum32[b] the fp32 sum,
 * sum64[b] the fp64 sum of the same values widened, bits_min[b] / bits_max[b] the unsigned minimum / maximum of their bit
 * patterns.  every_thread != 0: the flavour that leaves the result in every thread (read from the last one); 0: the thread-0
 * flavour. */
int     lrf_debug_block_reduce(const float* in, int32_t B, int32_t NT, int32_t every_thread, float* sum32, double* sum64,
                               uint32_t* bits_min, uint32_t* bits_max, void* stream);
void    lrf_debug_set_scene_fuse(int on);         /* lrf_scene_fwd: several fields per march / colour launch (default on); 0 = field by field */
void    lrf_debug_set_bwd_overlap(int on);        /* lrf_render_bwd: two branches on two streams (default on); 1 + 2 * (n + 1): k_wgrad_w2w3 on the caller's stream (n > 0, default) or on the side stream behind the density scatter (n = 0) */
void    lrf_debug_set_train_fwd_engine(int bits); /* 8: plane and line gradients by separate scatter kernels; 16: the gradient scatters with fp32 compare-and-swap adds (k_scatter_plane, rounds 2-5) instead of 64-bit fixed point (k_scatter_fix); 256: fixed point for the density tensors only (default: the appearance tensors too where their accumulators fit in LDS, lines up to 479 cells); 1024: no four-channel sweeps (lines of 480 .. 661 cells: the appearance tensors through the compare-and-swap kernel, as before); 512: k_wgrad_w2w3 in its single-buffered 128-row form (rounds 4-5) instead of the double-buffered 64-row one; 32 / 64 / 128: k_train_dgrad3 + k_train_app3 without their row stores / position gradient and X / dz1 products (timing experiments, wrong results) */
void    lrf_debug_set_scatter_wgs(int n);         /* lrf_render_bwd: workgroups of the binned plane / line scatter kernels (0 = default, one per CU); either mode -- the tests change the partition with it */
/* float offset of (row, col) inside the ACT (0) / GRD (1) region of a training workspace (MFMA-fragment order,
 * csrc/lrf_common.h); buffer 2: X-block column of appearance channel col.  Buffer 1, columns 48 .. 127, is the dX block in
 * its row-major order (what the compare-and-swap scatter kernels read); buffer 3: the same block in the groups order the
 * fixed-point appearance scatter asks for (lrf_debug_scatter_plan: appearance engine 0 or 1), col = 24 * plane + channel, 0 .. 71 */
int64_t lrf_debug_saved_row_offset(int buffer, uint64_t row, int col);
/* The gradient scatter engines lrf_render_bwd picks for a grid whose longest side is ll_max cells: a pure host function, no
 * device needed.  deterministic: LRF_FLAG_DETERMINISTIC; engine_bits: as lrf_debug_set_train_fwd_engine takes them (1 = the
 * defaults), or negative = whatever that switch holds now.  out = {density engine, appearance engine, density channels per
 * sweep, appearance channels per sweep, dynamic LDS bytes of the density scatter kernel, of the appearance scatter kernel, of
 * the density line kernel, of the appearance line kernel}; engines: 0 = int64 image (deterministic), 1 = 64-bit fixed point,
 * 2 = compare-and-swap with the lines fused, 3 = compare-and-swap with the lines apart (the line kernel runs only then).
 * Returns 0, 1 where lrf_render_bwd refuses the grid (deterministic and ll_max > 640), -1 for bad arguments. */
int     lrf_debug_scatter_plan(int32_t ll_max, int32_t deterministic, int32_t engine_bits, int64_t out[8]);
/* The launch plan of the forward render (csrc/lrf_forward.inl: plan_march, plan_shade3, pipe_chunks) for a field whose three
 * density lines are ll[0..2] cells long, R rays and S samples: a pure host function, no device needed.  switches: negative =
 * the process-wide hooks as they are set now; else bit 0 = density lines in LDS where they fit (lrf_debug_set_lds_lines),
 * bit 1 = tile offsets in LDS where they fit (lrf_debug_set_lds_toff), bits 2.. = lrf_debug_set_march_rays' value (0, 4, 8, 16).
 * out = {rays per k_march workgroup with the lines in LDS (0: lines from global memory), rays per group sum, z in LDS, k_march's
 * grid, block, dynamic LDS bytes, k_shade3's offsets in LDS, its dynamic LDS bytes, whether k_scan_tiles_n runs first, chunks of
 * the two-stream large-batch mode (1: one pass), the dynamic LDS k_march / k_shade3 are opted in for}.  Returns 0, -1 for bad
 * arguments (null, R <= 0, S outside 2 .. 4096, a line length <= 0, march rays not 0, 4, 8 or 16). */
int     lrf_debug_forward_plan(const int32_t ll[3], int32_t R, int32_t S, int32_t switches, int64_t out[12]);
/* Byte offsets, inside a training workspace (any flags: the deterministic mode's image lies behind everything else), of the two
 * words that hold the largest |contribution| of a backward as float bits: out[0] the density group's (k_bwd_ray), out[1] the
 * appearance group's (k_train_app3, written only where the appearance scatter runs on fixed point).  k_clear_bins zeroes both
 * in front of every backward; the fixed-point scatter kernels take their scale from them. */
void    lrf_debug_workspace_vmax_bwd(int32_t R, int32_t S, const int32_t grid[3], uint64_t out[2]);
/* k_depth_quantiles alone on caller-supplied weights w [R,S] (device), z [S], rays [R,6]; q: host [K], 1 <= K <= 4, each in
 * (0, 1] -> depth [K,R], index int32 [K,R] (nullable).  The arithmetic of csrc/lrf_quantile.inl without a forward render. */
int     lrf_depth_quantiles_from_weights(const float* w, const float* z, const float* rays, int32_t R, int32_t S, const float* q,
                                         int32_t K, float* depth, int32_t* index, void* stream);

/* lrf_mesh_vertex_normals (include/lrf.h) that also writes the integers behind the normals: S (device int64 [Nv,3]), the sum of
 * the fixed-point face normals around each vertex, and E (device int32 [1]), the exponent they share (INT32_MIN when every
 * face normal is zero). */
int     lrf_debug_mesh_vertex_normals(const float* vertices, const int32_t* faces, int64_t Nv, int64_t Nf, float* normals, int64_t* S,
                                      int32_t* E, int64_t* info, void* workspace, void* stream);

/* lrf_mesh_rasterize (include/lrf.h) with the tier threshold given: a (frame, face) pair whose pixel box holds at most small_max
 * pixels is walked by its own lane, a larger one by a wavefront.  0 sends every pair to the wavefronts, 2^31 - 1 every pair to
 * its lane; the outputs do not depend on it.  small_max < 0 is refused. */
int     lrf_debug_mesh_rasterize(const struct LrfMeshRaster* m,float* depth, int32_t* face, uint8_t* rgb8_out, float* weights,
                                 int32_t* crossings, int64_t* info, void* workspace, int32_t small_max, void* stream);

#ifdef __cplusplus
}
#endif
#endif
