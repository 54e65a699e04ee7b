// lrf_host.inl -- the host side that every entry point of the library shares (included by lrf_render.hip directly after
// lrf_common.h, so every .inl sees it): the error slot's one writer (refuse, set_err, LRF_HIP, LRF_TRY), the checked launch,
// the alignment test, the grid and size arithmetic and the workspace Carver.  No device code.
//
// The rule for an entry point ("Host side of an entry point"): its checks first, each refusal as
// refuse(who, "...") under one `const char* who`; its workspace through ONE carve function over a Carver, which its
// *_workspace_bytes calls over null and the entry point over the caller's buffer; every enqueue as LRF_TRY(launch(...)), the
// last one as `return launch(...)`.  The render path (launch_march, launch_shade3*, launch_shade_gen, render_fwd_impl,
// lrf_backward.inl, lrf_train32.inl, lrf_generic.inl, lrf_shade3*.inl) is the one exception: it enqueues raw and checks once per call.
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

}  // namespace lrf
