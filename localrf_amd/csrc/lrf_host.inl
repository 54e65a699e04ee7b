// lrf_host.inl -- the host side that every entry point of the library shares (included by lrf_render.hip directly after
// lrf_common.h, so every .inl sees it): the error slot's one writer (refuse, set_err, LRF_HIP, LRF_TRY), the checked launch,
// the alignment test, the grid and size arithmetic, the workspace Carver, the device's CU count and the side stream with its
// two-stream owner (TwoStreams).  No device code.
//
// The rule for an entry point ("Host side of an entry point"): its checks first, each refusal as
// refuse(who, "...") under one `const char* who`; its workspace through ONE carve function over a Carver, which its
// *_workspace_bytes calls over null and the entry point over the caller's buffer; every enqueue as LRF_TRY(launch(...)), the
// last one as `return launch(...)`.  The render path (lrf_forward.inl: sort_rays_if_asked, launch_march_k, launch_shade3*,
// launch_shade_gen, render_fwd_impl, which the fused groups of lrf_scene_fwd go through as well; lrf_backward.inl) is the one
// exception: it enqueues raw and checks once per call.
namespace lrf {

// the one writer of lrf_error_slot(): "<who>: <what>", or "<who>" alone; returns 1, so `return refuse(...)` refuses
static int refuse(const char* who, const char* what = nullptr) {
  snprintf(lrf_error_slot(), 512, "%s%s%s", who, what ? ": " : "", what ? what : "");
  return 1;
}
// a message that carries its own name, and the HIP error behind a failed call
static int set_err(const char* msg, hipError_t e = hipSuccess) { return refuse(msg, e != hipSuccess ? hipGetErrorString(e) : nullptr); }
#define LRF_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return set_err(#call, e_); } while (0)
#define LRF_TRY(call) do { if (int rc_ = (call)) return rc_; } while (0)     // a callee that has already set the error

static size_t round_up(size_t n, size_t to) { return (n + to - 1) / to * to; }
static unsigned blocks_for(long long n, int nt) { return (unsigned)((n + nt - 1) / nt); }

// any of the pointers (null passes) off the alignment mask + 1
template <class... P>
static bool misaligned(uintptr_t mask, const P*... p) { return ((uintptr_t)0 | ... | (uintptr_t)p) & mask; }

// enqueues k and checks the launch; used as LRF_TRY(launch(k, grid, nt, st, args...)), the arguments converted as by a call;
// launch_lds: with that many bytes of dynamic LDS
template <class... P, class... A>
static int launch_lds(void (*k)(P...), dim3 grid, int nt, size_t lds, hipStream_t st, const A&... args) {
  hipLaunchKernelGGL(k, grid, dim3(nt), lds, st, static_cast<P>(args)...);
  LRF_HIP(hipGetLastError());
  return 0;
}
template <class... P, class... A>
static int launch(void (*k)(P...), dim3 grid, int nt, hipStream_t st, const A&... args) {
  return launch_lds(k, grid, nt, 0, st, args...);
}

// a workspace layout is written once, as a function that takes its arrays from a Carver in order: over a null base it gives
// the size (bytes()), over the caller's workspace the pointers.  take(count) packs the pieces; take(count, 256) pads the piece
// to a multiple of 256 bytes, which keeps every piece of a layout 256-byte aligned whatever its neighbours hold (a double
// behind an odd number of floats).  A layout inside another is one piece of it: take<char>(inner bytes).
struct Carver {
  char* base;
  size_t at = 0;
  explicit Carver(void* ws) : base(static_cast<char*>(ws)) {}
  template <class T>
  T* take(size_t count, size_t align = 1) {
    T* p = reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(base) + at);
    at += round_up(count * sizeof(T), align);
    return p;
  }
  size_t bytes() const { return round_up(at, 256); }
};

// compute units of the current device: the grid of every persistent kernel
static int device_cus() {                 // of the current device (one process may drive several)
  static int cache[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  int& cus = cache[dev & 63];
  if (!cus) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    if (cus <= 0) cus = 256;
  }
  return cus;
}

// ---- Two streams for one call: host-only, shared by the forward (render_fwd_pipelined) and the backward (lrf_render_bwd)
static int g_bwd_overlap = 1;      // lrf_debug_set_bwd_overlap: weight-gradient GEMMs on a side stream, beside the scatter kernels
struct SideStream { hipStream_t s; hipEvent_t fork, join, app[2], bucket[5]; bool ok, bucket_set; std::mutex mu; };   // bucket[]: lrf_render_bwd_wait
static SideStream* side_stream() {
  static SideStream tab[64];
  static std::mutex init_mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  SideStream& x = tab[dev & 63];
  std::lock_guard<std::mutex> lk(init_mu);
  if (!x.ok) {
    if (hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    if (hipEventCreateWithFlags(&x.fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x.join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x.app[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x.app[1], hipEventDisableTiming) != hipSuccess) return nullptr;
    for (int q = 0; q < 5; ++q)
      if (hipEventCreateWithFlags(&x.bucket[q], hipEventDisableTiming) != hipSuccess) return nullptr;
    x.bucket_set = false;
    x.ok = true;
  }
  return &x;
}
// The caller's stream beside the device's side stream, for one call (lrf_render_bwd, render_fwd_pipelined).  Holds the
// SideStream's mutex for its lifetime: the side stream and its events are per device, so host threads that enqueue on the same
// device take turns (enqueueing a backward is ~0.3 ms of host time; the kernels themselves still overlap on the GPU).
// On one stream -- no SideStream, or (unless `always`) lrf_debug_set_bwd_overlap(0) or a capturing caller's stream -- side() is
// the caller's stream and fork / join / signal / wait do nothing.  The bucket events of lrf_render_bwd_wait are recorded
// whenever the device has a SideStream, on one stream and under capture too: that is sx against ss.
class TwoStreams {
  hipStream_t st;
  SideStream* sx;            // the device's, or null
  SideStream* ss;            // sx when the call runs on two streams, else null
  std::unique_lock<std::mutex> lock;
 public:
  explicit TwoStreams(hipStream_t caller, bool always = false) : st(caller), sx(side_stream()), ss(sx) {
    if (sx) lock = std::unique_lock<std::mutex>(sx->mu);
    if (ss && !always) {
      hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(st, &cap);
      if (!g_bwd_overlap || cap == hipStreamCaptureStatusActive) ss = nullptr;
    }
  }
  bool overlapping() const { return ss != nullptr; }
  hipStream_t side() const { return ss ? ss->s : st; }
  int fork() {               // the side stream continues from here
    if (ss) { LRF_HIP(hipEventRecord(ss->fork, st)); LRF_HIP(hipStreamWaitEvent(ss->s, ss->fork, 0)); }
    return 0;
  }
  int join() {               // the caller's stream continues behind everything on the side stream
    if (ss) { LRF_HIP(hipEventRecord(ss->join, ss->s)); LRF_HIP(hipStreamWaitEvent(st, ss->join, 0)); }
    return 0;
  }
  int signal(int i, hipStream_t s) { if (ss) LRF_HIP(hipEventRecord(ss->app[i], s)); return 0; }      // hand-off i (0, 1) is ready behind s ...
  int wait(int i, hipStream_t s) { if (ss) LRF_HIP(hipStreamWaitEvent(s, ss->app[i], 0)); return 0; } // ... and s goes on behind it
  int bucket(int i, hipStream_t s) { if (sx) LRF_HIP(hipEventRecord(sx->bucket[i], s)); return 0; }   // lrf_render_bwd_wait(i)'s event
  void finish() { if (sx) sx->bucket_set = true; }
};

}  // namespace lrf
