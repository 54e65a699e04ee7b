// lrf_forward.inl -- the host side of the forward render (included by lrf_render.hip behind the kernels, in front of
// lrf_backward.inl, whose training forward goes through the same helpers): workspace, test hooks, ray sorting, the launch plan
// of k_march and k_shade3 (pure host arithmetic, one place per rule), the launch helpers that take it, lrf_render_fwd.  No
// device code.  The render path enqueues raw (hipLaunchKernelGGL) and checks once per call: DESIGN.md 4v.
namespace lrf {

struct Workspace {
  int* toff; int* ncomp; float* acc; uint16_t* cidx; float* cw; float* part;
  int* gsum;               // k_march -> k_shade3: 32-sample tiles of each march workgroup's rays (at most ceil(R / 4) of them)
  float* rdir;             // k_march -> k_shade3: unit direction and length per ray
  int* perm; float* rays_s;  // ray sorting: slot -> ray, sorted copy of the rays
  int pmax; size_t bytes;
};
static Workspace carve(void* ws, int R, int S) {     // every piece padded to 256 bytes
  Workspace w;
  Carver c(ws);
  w.pmax = 2 * ((S + ITEM3 - 1) / ITEM3);             // partial slots per ray: enough for 16-sample tiles, 32-sample tiles and the training rows (two 16-row tiles per 32-sample tile)
  w.toff  = c.take<int>((size_t)R + 1, 256);
  w.ncomp = c.take<int>(R, 256);
  w.acc   = c.take<float>(R, 256);
  w.cidx  = c.take<uint16_t>((size_t)R * S, 256);     // (k_shade3 reads aligned dwords of it: an odd R * S ends 2 bytes short of a dword, inside the padding)
  w.cw    = c.take<float>((size_t)R * S, 256);
  w.part  = c.take<float>((size_t)R * w.pmax * 3, 256);
  w.rdir  = c.take<float>((size_t)R * 4, 256);
  w.perm  = c.take<int>(R, 256);
  w.rays_s = c.take<float>((size_t)R * 6, 256);
  w.gsum  = c.take<int>((R + 3) / 4, 256);
  w.bytes = c.bytes();
  return w;
}

// Test hooks (include/lrf_debug.h): process-wide, not part of the re-entrant ABI.
static float* g_dump = nullptr;    // lrf_debug_set_dump: device buffer for the s_memtime totals of k_shade3<TIMED>
static unsigned long long* g_march_dump = nullptr;   // lrf_debug_march_phases: device buffer [R][4] for the phase clocks of k_march_timed
static int g_no_lds_lines = 0;     // lrf_debug_set_lds_lines(0): k_march reads its lines from global memory
static int g_pipe_chunk = 16384;    // lrf_debug_set_pipe_chunk: rays per chunk of lrf_render_fwd's large-batch mode (0: one pass over the whole batch, as rounds 1-5)
static int g_march_rays = 0;       // lrf_debug_set_march_rays: rays per k_march workgroup (4, 8, 16) where that many fit; 0: plan_march's own choice
static int g_no_lds_toff = 0;      // lrf_debug_set_lds_toff(0): k_shade3 behind k_scan_tiles_n (global tile offsets) at every batch size
static int g_no_scene_fuse = 0;    // lrf_debug_set_scene_fuse(0): lrf_scene_fwd renders field by field (the tests compare the two forms)

// Dynamic LDS above 64 KB has to be opted into, once per device, before the first launch that asks for it: every render-path
// entry point calls this once its arguments are accepted (defined in lrf_render.hip behind every kernel it names).
static hipError_t lds_opt_in();

// LRF_FLAG_SORT_RAYS: sort the batch by direction (k_sort_rays) into the workspace; returns the rays the kernels should read
// and sets d.perm.  Batches beyond the 16-bit index of the sort words are rendered in the caller's order.
constexpr int LRF_SORT_MAX_R = 32768;
static bool sorts_rays(int R, uint32_t flags) { return (flags & LRF_FLAG_SORT_RAYS) && R >= 2 && R <= LRF_SORT_MAX_R; }
static const float* sort_rays_if_asked(DField& d, const float* rays, int R, uint32_t flags, const Workspace& w, hipStream_t st) {
  d.perm = nullptr;
  if (!sorts_rays(R, flags)) return rays;
  int N = 2;
  while (N < R) N <<= 1;
  hipLaunchKernelGGL(k_sort_rays, dim3(1), dim3(1024), (size_t)N * 4, st, rays, R, N, w.rays_s, w.perm);
  d.perm = w.perm;
  return w.rays_s;
}

// ---- The launch plan: what k_march and k_shade3 are launched with, as pure functions of the shapes and the hooks' switches.
// The three LDS budgets; lds_opt_in's table (lrf_render.hip) opts each kernel in for the most its plan can ask for.
constexpr size_t MARCH_LDS_BUDGET = 156 * 1024;                     // per CU, with the lines in LDS: 16 / nw workgroups' alpha slices + lines [+ z] (4 waves per SIMD either way)
constexpr size_t MARCH_LDS_OPT_IN = 160 * 1024;                     // ... and what k_march<true> is opted in for: one 16-ray workgroup with z and the tail
constexpr size_t MARCH_LDS_NOLINES = 64 * 1024 + MARCH_LDS_TAIL;    // per workgroup of k_march<false>: four alpha slices [+ z] and the tail
constexpr size_t SHADE3_LDS_CAP = 160 * 1024 - 256;                 // per workgroup of the colour kernel (one per CU; 256 B of static LDS)
constexpr int SHADE3_MAX_GROUPS = 512 * TILE_GPT;                   // group sums one workgroup of the colour kernel holds in registers

// k_march: rays per workgroup with the density lines in LDS (nw = 4, 8 or 16: 4 / 2 / 1 workgroups per CU, whichever keeps
// alpha slices + lines inside the budget -- 300^3: 8 + 29 KB x 4; 500^3: 18 + 48 KB x 2; 640^3: 47 + 61 KB x 1), or nw = 0:
// k_march<false> reads the lines from global memory, 4 rays per workgroup (grids of about 900^3 and above, or lds_lines
// off).  march_rays (test hook): a larger nw than the smallest that fits.  zlds: the schedule's S floats join in LDS where the
// same budget still holds with them (300^3 at S = 512: (8 + 28.8 + 2 KB) x 4 = 155.2 KB).  group: the unit of Workspace::gsum.
struct MarchPlan { int nw, group, zlds; unsigned grid, block; size_t lds; };
static MarchPlan plan_march(const int32_t ll[3], int R, int S, bool lds_lines, int march_rays) {
  const size_t slice = (size_t)S * sizeof(float), lds_l = (size_t)(ll[0] + ll[1] + ll[2]) * LRF_CD * sizeof(float);
  MarchPlan m{};
  for (int cand = 4; lds_lines && cand <= 16; cand *= 2)
    if ((cand * slice + lds_l) * (16 / cand) <= MARCH_LDS_BUDGET) {
      if (!m.nw) m.nw = cand;
      if (cand == march_rays) { m.nw = cand; break; }
    }
  m.group = m.nw ? m.nw : 4;
  m.zlds = m.nw ? ((m.nw + 1) * slice + lds_l) * (16 / m.nw) <= MARCH_LDS_BUDGET : 5 * slice + MARCH_LDS_TAIL <= MARCH_LDS_NOLINES;
  m.grid = (unsigned)((R + m.group - 1) / m.group);
  m.block = 64u * m.group;
  m.lds = m.group * slice + (m.nw ? lds_l : 0) + (m.zlds ? slice : 0) + MARCH_LDS_TAIL;
  return m;
}
static MarchPlan plan_march(const int32_t ll[3], int R, int S) { return plan_march(ll, R, S, !g_no_lds_lines, g_march_rays); }
static_assert(MARCH_LDS_BUDGET + MARCH_LDS_TAIL <= MARCH_LDS_OPT_IN, "a 16-ray workgroup of k_march<true> stays inside its opt-in");

// k_shade3: its tile offsets are built in the kernel from k_march's group sums when R + 1 offsets and R 16-bit counts (absolute
// ray index; a workgroup fills only its own window) fit in LDS beside image and z, and there are no more group sums than one
// workgroup holds in registers; else k_scan_tiles_n runs first and the kernel reads global offsets.
static size_t shade3_toff_lds(int R) { return (size_t)(R + 1) * sizeof(int) + (size_t)R * sizeof(unsigned short) + 16; }
struct Shade3Plan { bool in_lds; size_t lds_base, lds_toff, lds; };
static Shade3Plan plan_shade3(int R, int S, int group_rays, bool lds_toff) {
  Shade3Plan p;
  p.lds_base = (size_t)W32_ALL_U4 * sizeof(uint4) + (size_t)S * sizeof(float);
  p.lds_toff = shade3_toff_lds(R);
  p.in_lds = lds_toff && p.lds_base + p.lds_toff + 64 <= SHADE3_LDS_CAP && (R + group_rays - 1) / group_rays <= SHADE3_MAX_GROUPS;
  p.lds = p.lds_base + (p.in_lds ? p.lds_toff : 0);
  return p;
}
static_assert((size_t)W32_ALL_U4 * sizeof(uint4) + 4096 * sizeof(float) <= SHADE3_LDS_CAP, "image + z of the largest S: the forms without offsets in LDS");

// What k_march reads and writes besides the field, the rays and the schedule
struct MarchIO { float* depth; float* acc; float* w_all; int* ncomp; int* gsum; uint16_t* cidx; float* cw; float* feat; };
// ... into workspace w: the caller's depth, optional weights [R,S] and feature rows [R,S]; group_sums: for k_shade3's in-kernel
// offsets (the engines that scan the counts themselves take none)
static MarchIO march_io(const Workspace& w, float* depth, float* w_all, float* feat, bool group_sums = true) {
  return MarchIO{depth, w.acc, w_all, w.ncomp, group_sums ? w.gsum : nullptr, w.cidx, w.cw, feat};
}

// the one launch line of k_march: every kernel of the family takes (field or fields, ..., zlds) and the plan's shape
template <class K, class F>
static void launch_march_k(K k, const MarchPlan& m, const F& f, const float* rays, const float* z, int R, int S, uint32_t flags, float floater,
                           const MarchIO& io, hipStream_t st) {
  hipLaunchKernelGGL(k, dim3(m.grid), dim3(m.block), m.lds, st,
                     f, rays, z, R, S, flags, floater, io.depth, io.acc, io.w_all, io.ncomp, io.gsum, io.cidx, io.cw, io.feat, m.zlds);
}
// k_march over one field; with lrf_debug_march_phases' buffer set, the timed kernel (phase clocks -> the dump buffer)
static void launch_march(const MarchPlan& m, const DField& d, const float* rays, const float* z, int R, int S, uint32_t flags, float floater,
                         const MarchIO& io, hipStream_t st) {
  if (g_march_dump) {
    DField dt = d;
    dt.dump = reinterpret_cast<float*>(g_march_dump);
    return launch_march_k(m.nw ? k_march_timed<true> : k_march_timed<false>, m, dt, rays, z, R, S, flags, floater, io, st);
  }
  launch_march_k(m.nw ? k_march<true> : k_march<false>, m, d, rays, z, R, S, flags, floater, io, st);
}
// ... over the fused fields of a scene: this form exists with the lines in LDS only (scene_fuses refuses m.nw == 0), and the
// caller made sure that Rf is a multiple of 16 >= nw
static void launch_march(const MarchPlan& m, const MultiF& mf, const float* rays, const float* z, int R, int S, uint32_t flags, float floater,
                         const MarchIO& io, hipStream_t st) {
  launch_march_k(k_march<true, true>, m, mf, rays, z, R, S, flags, floater, io, st);
}

// k_march's output -> colours: k_shade3 over w.gsum (group_rays rays per entry, as the march plan left them) or, where the plan
// says so, behind k_scan_tiles_n over toff32 (R + 1 ints).  sv == nullptr: the eval forward; else the training forward, which
// also leaves the rows of SaveOut3 (and sv->toff16 must not be toff32).  dump: lrf_debug_set_dump's buffer (eval only, and only
// with the offsets in LDS).
static void launch_shade3(DField d, const float* rays, const float* z, int R, int S, uint32_t flags, const Workspace& w, int group_rays,
                         int* toff32, float* rgb, float* acc_out, const SaveOut3* sv, float* dump, hipStream_t st) {
  const Shade3Plan p = plan_shade3(R, S, group_rays, !g_no_lds_toff);
  const bool timed = !sv && p.in_lds && dump;                 // test hook: phase timing, s_memtime totals -> the dump buffer
  if (timed) d.dump = dump;
  if (!p.in_lds) hipLaunchKernelGGL(k_scan_tiles_n<ITEM3>, dim3(1), dim3(1024), 0, st, w.ncomp, R, toff32);
  auto k = sv ? (p.in_lds ? k_shade3<8, true, false, true> : k_shade3<8, false, false, true>)
              : (timed ? k_shade3<8, true, true> : p.in_lds ? k_shade3<8, true, false> : k_shade3<8, false, false>);
  hipLaunchKernelGGL(k, dim3(device_cus()), dim3(512), p.lds, st,
                     d, rays, z, S, p.in_lds ? w.gsum : toff32, R, w.ncomp, w.cidx, w.cw, w.part, w.pmax, flags, w.acc, rgb, acc_out,
                     sv ? *sv : SaveOut3{}, group_rays);
}

// Several fields, one launch (see MultiF): global tile offsets over all virtual rays (k_scan_tiles_n), then the colour kernel.
static void launch_shade3_multi(const MultiF& mf, const float* rays, const float* z, int Rv, int S, uint32_t flags,
                                const Workspace& w, float* rgb, hipStream_t st) {
  const Shade3Plan p = plan_shade3(Rv, S, 4, false);
  hipLaunchKernelGGL(k_scan_tiles_n<ITEM3>, dim3(1), dim3(1024), 0, st, w.ncomp, Rv, w.toff);
  hipLaunchKernelGGL((k_shade3m<8, false>), dim3(device_cus()), dim3(512), p.lds, st,
                     mf, rays, z, S, w.toff, Rv, w.ncomp, w.cidx, w.cw, w.part, w.pmax, flags, w.acc, rgb, (float*)nullptr, SaveOut3{}, 0);
}

// network configuration of a field: null, or why it cannot be rendered
static const char* gen_check(const LrfField* f) {
  const int fc = f->feature_c ? f->feature_c : LRF_FEATC;
  if (f->fea_pe < 0 || f->fea_pe > GEN_MAX_PE || f->view_pe < 0 || f->view_pe > GEN_MAX_PE || fc < 1 || fc > GEN_MAX_FC)
    return "localrf: unsupported colour-network configuration (need 0 <= fea_pe, view_pe <= 6 and 1 <= featureC <= 256)";
  if (!gen_is_default(f->fea_pe, f->view_pe, fc) && (!f->basis || !f->w1 || !f->b1 || !f->w2 || !f->b2 || !f->w3 || !f->b3))
    return "localrf: a non-default colour-network configuration needs the natural-layout weights in LrfField (basis, w1 .. b3)";
  return nullptr;
}
// the generic colour kernel behind k_march; toff32 != null: the training forward (also leaves colours, feat rows, tile records)
static hipError_t launch_shade_gen(const DField& d, const GenCfg& gc, const float* rays, const float* z, int R, int S, const Workspace& w,
                                   const int* toff32, float* crgb, float* act, int4* tileinfo, hipStream_t st) {
  constexpr int ls = 32;                                      // (the forward's LDS image is at most ~116 KB (fea_pe = view_pe = 6, feature_c = 256), under the 159 KB opt-in)
  const int nt = gen_block_threads(gc);
  const size_t lds = (size_t)gen_lds(gc, ls, false).total * 4;
  const dim3 grid(R * ((w.pmax * 16 + ls - 1) / ls));
  auto k = toff32 ? k_shade_gen<32, true> : k_shade_gen<32, false>;
  hipLaunchKernelGGL(k, grid, dim3(nt), lds, st, d, gc, rays, z, S, w.ncomp, w.cidx, w.cw, w.part, w.pmax, toff32, crgb, act, tileinfo);
  return hipGetLastError();
}

// Large batches (full-frame evaluation: renderer.py:65-77 renders an image 4096 rays at a time) go through the two kernels
// in chunks of g_pipe_chunk rays that alternate over the caller's stream and the side stream: a chunk's k_march and the
// tail of its k_shade3 run beside the other stream's colour kernel (k_shade3 is one persistent workgroup per CU bound by
// instruction issue at 46 %; k_march is latency / L2 bound).  65536 rays at configs[1]: 2.38 ms in one pass, 2.49 / 2.30 /
// 2.24 / 2.26 / 2.30 ms in chunks of 4096 / 8192 / 16384 / 24576 / 32768 (scripts/pipe_chunk_probe.py; 262144 rays: 9.55 ->
// 8.69 ms = 30.2 M rays/s); below two chunks of 16384 one pass is as fast or faster.  Every chunk has a workspace of its own
// inside the caller's.
static int pipe_chunks(int R) { return (g_pipe_chunk > 0 && R >= 2 * g_pipe_chunk) ? (R + g_pipe_chunk - 1) / g_pipe_chunk : 1; }

// the colour network the split-bf16 kernels are built for: fea_pe = view_pe = 0, featureC = 128
static bool default_net(const LrfField* f) { return gen_is_default(f->fea_pe, f->view_pe, f->feature_c ? f->feature_c : LRF_FEATC); }
// Every refusal of the forward render, before anything is enqueued; null when the batch can be rendered.
static const char* check_fwd(const LrfField* f, const float* rays, const float* z, const float* rgb, const float* depth,
                             const void* workspace, int32_t R, int32_t S, uint32_t flags) {
  if (!f || !f->cache || !rays || !z || !rgb || !depth || !workspace) return "lrf_render_fwd: null argument";
  if (R <= 0 || S < 2 || S > 4096) return "lrf_render_fwd: need R > 0 and 2 <= S <= 4096";
  if (flags & ~(LRF_FLAG_ALL & ~(LRF_FLAG_ROWS_SAVED | LRF_FLAG_PLANE_EVENTS))) return "lrf_render_fwd: unknown flag bits (caller built against another ABI version?)";
  if (const char* bad = gen_check(f)) return bad;
  if (!default_net(f) && (flags & LRF_FLAG_MLP_F32))
    return "lrf_render_fwd: the exact-fp32 MFMA engine is built for fea_pe = view_pe = 0, featureC = 128 only";
  return nullptr;
}
// the default engine: k_march -> k_shade3, two launches and no finalize kernel
static bool fwd_shade3(const LrfField* f, uint32_t flags) { return default_net(f) && !(flags & (LRF_FLAG_MLP_VALU | LRF_FLAG_MLP_F32)); }

// One batch of rays (accepted by check_fwd) through k_march and the colour stage on `st`; ev (optional,
// lrf_render_fwd_profile): 4 events = start, after k_march, after the colour kernel(s), end.
static int render_fwd_impl(const LrfField* f, const float* rays, const float* z, int32_t R, int32_t S,
                           uint32_t flags, float floater_thresh, float* rgb, float* depth,
                           float* weight_out, float* acc_out, void* workspace, hipStream_t st, hipEvent_t* ev) {
  DField d = make_dfield(f);
  const Workspace w = carve(workspace, R, S);
  const MarchPlan m = plan_march(d.ll, R, S);
  const bool shade3 = fwd_shade3(f, flags);
  if (ev) LRF_HIP(hipEventRecord(ev[0], st));
  rays = sort_rays_if_asked(d, rays, R, flags, w, st);
  if (shade3) d.rdir = w.rdir;
  launch_march(m, d, rays, z, R, S, flags, floater_thresh, march_io(w, depth, weight_out, nullptr, shade3), st);
  if (ev) LRF_HIP(hipEventRecord(ev[1], st));
  if (shade3) {
    // Default engine: k_march -> k_shade3 (32 samples per wave on v_mfma_f32_32x32x16_bf16, lrf_shade3.inl); the tile
    // offsets are built inside the colour kernel from k_march's group sums (w.gsum) when they fit in LDS beside the image,
    // scanned by k_scan_tiles_n otherwise.
    launch_shade3(d, rays, z, R, S, flags, w, m.group, w.toff, rgb, acc_out, nullptr, g_dump, st);
    if (ev) { LRF_HIP(hipEventRecord(ev[2], st)); LRF_HIP(hipEventRecord(ev[3], st)); }
    LRF_HIP(hipGetLastError());
    return 0;
  }
  // exact-fp32 / plain-loop engines: 16-sample tiles and no group sums (they scan the counts): [k_scan_tiles ->] colour kernel -> k_finalize
  if (!default_net(f) || (flags & LRF_FLAG_MLP_VALU)) {
    const GenCfg gc = gen_cfg(d.fea_pe, d.view_pe, d.fc, !(flags & LRF_FLAG_PE_OFF));
    LRF_HIP(launch_shade_gen(d, gc, rays, z, R, S, w, nullptr, nullptr, nullptr, nullptr, st));
  } else {
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, st, w.ncomp, R, w.toff);
    hipLaunchKernelGGL(k_shade, dim3(device_cus()), dim3(1024), 0, st, d, rays, z, S, w.toff, R, w.ncomp, w.cidx, w.cw, w.part, w.pmax);
  }
  if (ev) LRF_HIP(hipEventRecord(ev[2], st));
  hipLaunchKernelGGL(k_finalize, dim3((R + 255) / 256), dim3(256), 0, st, R, w.pmax, flags, w.ncomp, w.acc, w.part, rgb, acc_out, d.perm);
  if (ev) LRF_HIP(hipEventRecord(ev[3], st));
  LRF_HIP(hipGetLastError());
  return 0;
}

// render_fwd_impl, large batches in chunks over two streams (see pipe_chunks); 0 or an error code
static int render_fwd_pipelined(const LrfField* f, const float* rays, const float* z, int32_t R, int32_t S,
                                uint32_t flags, float floater_thresh, float* rgb, float* depth,
                                float* weight_out, float* acc_out, void* workspace, hipStream_t st) {
  const int nc = pipe_chunks(R);
  if (nc <= 1) return render_fwd_impl(f, rays, z, R, S, flags, floater_thresh, rgb, depth, weight_out, acc_out, workspace, st, nullptr);
  TwoStreams ts(st, true);
  if (!ts.overlapping()) return render_fwd_impl(f, rays, z, R, S, flags, floater_thresh, rgb, depth, weight_out, acc_out, workspace, st, nullptr);
  LRF_TRY(ts.fork());
  const size_t wb = carve(nullptr, g_pipe_chunk, S).bytes;
  int rc = 0;
  for (int c = 0; c < nc && rc == 0; ++c) {
    const int r0 = c * g_pipe_chunk, rn = std::min(g_pipe_chunk, R - r0);
    rc = render_fwd_impl(f, rays + (size_t)r0 * 6, z, rn, S, flags, floater_thresh, rgb + (size_t)r0 * 3, depth + r0,
                         weight_out ? weight_out + (size_t)r0 * S : nullptr, acc_out ? acc_out + r0 : nullptr,
                         static_cast<char*>(workspace) + (size_t)c * wb, (c & 1) ? ts.side() : st, nullptr);
  }
  LRF_TRY(ts.join());                                       // (also after an error: the side stream is joined again)
  return rc;
}

}  // namespace lrf

extern "C" size_t lrf_workspace_bytes(int32_t R, int32_t S) {
  using namespace lrf;
  const size_t whole = carve(nullptr, R, S).bytes;
  const int nc = pipe_chunks(R);
  return nc > 1 ? std::max(whole, (size_t)nc * carve(nullptr, g_pipe_chunk, S).bytes) : whole;
}

extern "C" int lrf_render_fwd(const LrfField* f, const float* rays, const float* z, int32_t R, int32_t S,
                              uint32_t flags, float floater_thresh, float* rgb, float* depth,
                              float* weight_out, float* acc_out, void* workspace, void* stream) {
  using namespace lrf;
  if (const char* bad = check_fwd(f, rays, z, rgb, depth, workspace, R, S, flags)) return set_err(bad);
  LRF_HIP(lds_opt_in());
  return render_fwd_pipelined(f, rays, z, R, S, flags, floater_thresh, rgb, depth, weight_out, acc_out, workspace,
                              reinterpret_cast<hipStream_t>(stream));
}

extern "C" int lrf_render_fwd_profile(const LrfField* f, const float* rays, const float* z, int32_t R, int32_t S,
                                      uint32_t flags, float floater_thresh, float* rgb, float* depth,
                                      void* workspace, void* stream, float* ms_out, int32_t* n_shaded_out) {
  using namespace lrf;
  if (!ms_out) return set_err("lrf_render_fwd_profile: null ms_out");
  if (const char* bad = check_fwd(f, rays, z, rgb, depth, workspace, R, S, flags)) return set_err(bad);
  LRF_HIP(lds_opt_in());
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipEvent_t ev[4];
  for (int i = 0; i < 4; ++i) LRF_HIP(hipEventCreate(&ev[i]));
  int rc = render_fwd_impl(f, rays, z, R, S, flags, floater_thresh, rgb, depth, nullptr, nullptr, workspace, st, ev);
  if (rc == 0) {
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = set_err("hipStreamSynchronize", e);
  }
  if (rc == 0) {
    for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]);      // march, colour stage, finalize (0 for the default engine)
    (void)hipEventElapsedTime(&ms_out[3], ev[0], ev[3]);
    if (fwd_shade3(f, flags)) { ms_out[2] = 0.0f; (void)hipEventElapsedTime(&ms_out[3], ev[0], ev[2]); }
    ms_out[4] = ms_out[5] = 0.0f;
    if (n_shaded_out) {
      // shaded-sample count of this batch = sum of ncomp (host copy; measurement only)
      const Workspace w = carve(workspace, R, S);
      int* h = (int*)malloc((size_t)R * sizeof(int));
      if (h && hipMemcpy(h, w.ncomp, (size_t)R * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) {
        long long tot = 0; for (int i = 0; i < R; ++i) tot += h[i];
        *n_shaded_out = (int32_t)tot;
      }
      free(h);
    }
  }
  for (int i = 0; i < 4; ++i) (void)hipEventDestroy(ev[i]);
  return rc;
}

// The forward's launch plan as lrf_render_fwd would form it, for a CPU test (include/lrf_debug.h): no device needed.
extern "C" int lrf_debug_forward_plan(const int32_t ll[3], int32_t R, int32_t S, int32_t switches, int64_t out[12]) {
  using namespace lrf;
  if (!ll || !out || R <= 0 || S < 2 || S > 4096 || ll[0] <= 0 || ll[1] <= 0 || ll[2] <= 0) return -1;
  const bool hooks = switches < 0;
  const int rays = hooks ? g_march_rays : switches >> 2;
  if (rays != 0 && rays != 4 && rays != 8 && rays != 16) return -1;
  const MarchPlan m = plan_march(ll, R, S, hooks ? !g_no_lds_lines : (switches & 1) != 0, rays);
  const Shade3Plan p = plan_shade3(R, S, m.group, hooks ? !g_no_lds_toff : (switches & 2) != 0);
  const int64_t v[12] = {m.nw, m.group, m.zlds, m.grid, m.block, (int64_t)m.lds, p.in_lds, (int64_t)p.lds, !p.in_lds, pipe_chunks(R),
                         (int64_t)(m.nw ? MARCH_LDS_OPT_IN : MARCH_LDS_NOLINES), (int64_t)SHADE3_LDS_CAP};
  for (int i = 0; i < 12; ++i) out[i] = v[i];
  return 0;
}
