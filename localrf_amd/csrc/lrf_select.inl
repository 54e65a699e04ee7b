// lrf_select.inl -- exact order statistics of B fp32 rows on the device (included by lrf_render.hip):
//   LRF_SELECT_QUANTILE  np.quantile(row, q) with numpy's default method="linear", bit for bit (numpy 2.2 arithmetic below)
//   LRF_SELECT_MEDIAN    torch.median(row): the element of rank floor((n - 1) / 2)
//
// Radix select, most significant digit first.  Every value maps to an order-preserving uint32 key (positives: sign bit
// set; negatives: all bits flipped; -0.0 is read as +0.0, so the two compare equal and a zero result is +0.0; every NaN
// maps to 0xFFFFFFFF, after +inf, as numpy sorts it).  Four passes of 8-bit digits: k_select_hist counts the digits of
// the keys that match the digits fixed so far into an LDS histogram (integer atomics), then adds each non-zero bin to the
// row's global histogram once per workgroup; k_select_scan (one workgroup per row) scans the 256 bins and fixes the digit
// and the remaining rank.  After pass 4 the key of rank lo is known, and with it how many keys equal it: rank lo + 1 is
// either the same key or the smallest key above it, which k_select_min finds in one more pass (integer atomicMin) only
// for the rows that need it.  k_select_finish forms the result.  Integer atomics only, no host synchronisation, a fixed
// sequence of 11 launches: capturable in a hipGraph and bit-reproducible by construction.
//
// numpy's linear quantile of a float32 array (numpy/lib/_function_base_impl.py: _compute_virtual_index, _get_indexes,
// _get_gamma, _lerp), restated exactly:
//   q is rounded to fp32; v = fp32(fp32(n - 1) * q);
//   v >= n - 1: lo = hi = n - 1 and prev = -1 (numpy overwrites the floor with -1 and still takes gamma from it),
//   else prev = floor(v), lo = prev, hi = lo + 1;
//   t = fp32(v - prev); d = x[hi] - x[lo];  result = t >= 0.5 ? x[hi] - d * (1 - t) : x[lo] + d * t   (fp32, unfused:
//   the kernels that do this arithmetic turn contraction off);
//   a row holding a NaN gives NaN.  The inf - inf of d makes NaN wherever numpy's does.
namespace lrf {

constexpr int SEL_NT = 256;
constexpr int SEL_ITEMS = 16;
constexpr int SEL_CHUNK = SEL_NT * SEL_ITEMS;    // values per workgroup per pass

struct SelRow {                  // per-row state in the workspace
  long long n;
  unsigned prefix;               // key digits fixed so far (rank lo)
  unsigned rem;                  // rank of the target among the keys that match prefix
  unsigned want_hi;              // 1: the result also needs rank lo + 1
  unsigned need_min;             // 1: rank lo + 1 is the smallest key above the rank-lo key
  unsigned min_above;            // that key (k_select_min)
  unsigned nan;                  // the row holds a NaN
  float gamma;
  unsigned pad[3];
};
static_assert(sizeof(SelRow) == 48, "SelRow layout");

struct SelectInit {
  int B, uniform, mode;
  float q;
  long long n[LRF_SELECT_MAX_ROWS];
};

__device__ __forceinline__ unsigned sel_key(float v) {
  unsigned u = __float_as_uint(v);
  if (v != v) return 0xFFFFFFFFu;
  if (u == 0x80000000u) u = 0u;                                    // -0.0 == +0.0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_value(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// [B rows] [B x 4 passes x 256 bins]
struct SelectWs { SelRow* rows; unsigned* hist; size_t bytes; };
static SelectWs carve_select(void* ws, int B) {
  SelectWs w;
  Carver c(ws);
  w.rows = c.take<SelRow>(B);
  w.hist = c.take<unsigned>((size_t)B * 4 * 256);
  w.bytes = c.bytes();
  return w;
}
static size_t select_ws_bytes(int B) { return carve_select(nullptr, B).bytes; }

__global__ __launch_bounds__(SEL_NT) void k_select_init(SelectInit a, SelRow* __restrict__ rows, unsigned* __restrict__ hist) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < 4 * 256; i += SEL_NT) hist[(size_t)b * 1024 + i] = 0u;
  if (tid != 0) return;
  const long long n = a.n[a.uniform ? 0 : b];
  long long lo;
  SelRow r;
  r.n = n; r.prefix = 0u; r.want_hi = 0u; r.need_min = 0u; r.min_above = 0xFFFFFFFFu; r.nan = 0u; r.gamma = 0.0f;
  if (a.mode == LRF_SELECT_MEDIAN) {
    lo = (n - 1) / 2;
  } else {
    const float nm1 = (float)(n - 1);
    const float v = nm1 * a.q;
    float prev;
    if (v >= nm1) { lo = n - 1; prev = -1.0f; }
    else { prev = floorf(v); lo = (long long)prev; r.want_hi = 1u; }
    r.gamma = (float)((double)v - (double)prev);
  }
  r.rem = (unsigned)lo;
  for (int k = 0; k < 3; ++k) r.pad[k] = 0u;
  rows[b] = r;
}

__global__ __launch_bounds__(SEL_NT) void k_select_hist(const float* __restrict__ x, long long stride, SelRow* __restrict__ rows,
                                                        unsigned* __restrict__ hist, int pass) {
  __shared__ unsigned h[256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const long long n = rows[b].n;
  const long long base = (long long)blockIdx.x * SEL_CHUNK;
  if (base >= n) return;                                           // uniform over the workgroup
  const int shift = 24 - 8 * pass;
  const unsigned mask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
  const unsigned prefix = rows[b].prefix;
  h[tid] = 0u;
  __syncthreads();
  const float* p = x + (size_t)b * stride;
  int any_nan = 0;
#pragma unroll 4
  for (int k = 0; k < SEL_ITEMS; ++k) {
    const long long i = base + (long long)k * SEL_NT + tid;
    if (i < n) {
      const float v = p[i];
      any_nan |= v != v;
      const unsigned key = sel_key(v);
      if ((key & mask) == prefix) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
  }
  if (pass == 0 && __syncthreads_or(any_nan)) {
    if (tid == 0) atomicOr(&rows[b].nan, 1u);
  }
  __syncthreads();
  const unsigned c = h[tid];
  if (c) atomicAdd(&hist[((size_t)b * 4 + pass) * 256 + tid], c);
}

// one workgroup per row: inclusive scan of the pass's 256 bins; the bin holding rank `rem` fixes the digit
__global__ __launch_bounds__(SEL_NT) void k_select_scan(SelRow* __restrict__ rows, const unsigned* __restrict__ hist, int pass) {
  __shared__ unsigned s[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned rem = rows[b].rem;
  const unsigned c = hist[((size_t)b * 4 + pass) * 256 + tid];
  s[tid] = c;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const unsigned t = tid >= off ? s[tid - off] : 0u;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  const unsigned incl = s[tid], excl = incl - c;
  if (c != 0u && excl <= rem && rem < incl) {                      // exactly one thread
    SelRow& r = rows[b];
    r.prefix |= (unsigned)tid << (24 - 8 * pass);
    r.rem = rem - excl;
    if (pass == 3) r.need_min = (r.want_hi && rem - excl + 1u >= c) ? 1u : 0u;   // rank lo + 1 lies above this key
  }
}

// the smallest key above the rank-lo key, for the rows whose rank lo + 1 is not a copy of it
__global__ __launch_bounds__(SEL_NT) void k_select_min(const float* __restrict__ x, long long stride, SelRow* __restrict__ rows) {
  __shared__ unsigned red[SEL_NT / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (!rows[b].need_min) return;
  const long long n = rows[b].n;
  const long long base = (long long)blockIdx.x * SEL_CHUNK;
  if (base >= n) return;
  const unsigned key_lo = rows[b].prefix;
  const float* p = x + (size_t)b * stride;
  unsigned m = 0xFFFFFFFFu;
#pragma unroll 4
  for (int k = 0; k < SEL_ITEMS; ++k) {
    const long long i = base + (long long)k * SEL_NT + tid;
    if (i < n) {
      const unsigned key = sel_key(p[i]);
      if (key > key_lo && key < m) m = key;
    }
  }
  // block_min0's order by hand: with the helper the largest quantile of geometry_probe.py took 0.21 ms against 0.19 (docs/REDUCE_HELPERS_FIGURES.md)
  for (int off = 32; off > 0; off >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < SEL_NT / 64; ++w) m = min(m, red[w]);
    if (m != 0xFFFFFFFFu) atomicMin(&rows[b].min_above, m);
  }
}

__global__ __launch_bounds__(SEL_NT) void k_select_finish(const SelRow* __restrict__ rows, int B, int mode, float* __restrict__ out) {
#pragma clang fp contract(off)       // numpy rounds the product before the sum (hip's __fmul_rn is a plain, fusable multiply)
  const int b = blockIdx.x * SEL_NT + threadIdx.x;
  if (b >= B) return;
  const SelRow r = rows[b];
  const float a = sel_value(r.prefix);
  float res = a;
  if (mode == LRF_SELECT_QUANTILE) {
    const float hi = r.need_min ? sel_value(r.min_above) : a;
    const float t = r.gamma;
    const float d = hi - a;
    res = t >= 0.5f ? hi - d * (1.0f - t) : a + d * t;
  }
  if (r.nan) res = __uint_as_float(0x7FC00000u);
  out[b] = res;
}

// the whole sequence; arguments already checked.  n: host array of B lengths, or of one when uniform.
static int select_launch(const float* x, long long stride, const int64_t* n, int uniform, int B, int mode, float q, float* out,
                         void* workspace, hipStream_t st) {
  SelectInit a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.uniform = uniform; a.mode = mode; a.q = q;
  long long max_n = 0;
  for (int b = 0; b < (uniform ? 1 : B); ++b) { a.n[b] = n[b]; max_n = n[b] > max_n ? n[b] : max_n; }
  const SelectWs w = carve_select(workspace, B);
  const unsigned chunks = blocks_for(max_n, SEL_CHUNK);
  LRF_TRY(launch(k_select_init, B, SEL_NT, st, a, w.rows, w.hist));
  for (int pass = 0; pass < 4; ++pass) {
    LRF_TRY(launch(k_select_hist, dim3(chunks, B), SEL_NT, st, x, stride, w.rows, w.hist, pass));
    LRF_TRY(launch(k_select_scan, B, SEL_NT, st, w.rows, w.hist, pass));
  }
  if (mode == LRF_SELECT_QUANTILE) LRF_TRY(launch(k_select_min, dim3(chunks, B), SEL_NT, st, x, stride, w.rows));
  return launch(k_select_finish, blocks_for(B, SEL_NT), SEL_NT, st, w.rows, B, mode, out);
}

static bool select_n_ok(long long n) { return n >= 1 && n < (1ll << 31); }

}  // namespace lrf

extern "C" size_t lrf_select_workspace_bytes(int32_t B, int64_t max_n) {
  if (B < 1 || B > 65535 || !lrf::select_n_ok(max_n)) return 0;
  return lrf::select_ws_bytes(B);
}

extern "C" int lrf_select(const float* x, int64_t row_stride, const int64_t* n, int32_t n_count, int32_t B, int32_t mode, float q,
                          float* out, void* workspace, void* stream) {
  using namespace lrf;
  const char* who = "lrf_select";
  if (!x || !n || !out || !workspace) return refuse(who, "null argument");
  if (B < 1 || B > 65535) return refuse(who, "need 1 <= B <= 65535");
  if (n_count != 1 && n_count != B) return refuse(who, "n_count must be 1 (equal rows) or B");
  if (n_count != 1 && B > LRF_SELECT_MAX_ROWS) return refuse(who, "rows of individual lengths are limited to LRF_SELECT_MAX_ROWS");
  for (int b = 0; b < n_count; ++b)
    if (!select_n_ok(n[b])) return refuse(who, "every row length n must satisfy 1 <= n < 2^31");
  if (row_stride < 0) return refuse(who, "row_stride must be >= 0");
  if (mode != LRF_SELECT_QUANTILE && mode != LRF_SELECT_MEDIAN) return refuse(who, "mode must be LRF_SELECT_QUANTILE or LRF_SELECT_MEDIAN");
  if (mode == LRF_SELECT_QUANTILE && !(q >= 0.0f && q <= 1.0f)) return refuse(who, "q must lie in [0, 1]");
  return select_launch(x, row_stride, n, n_count == 1, B, mode, q, out, workspace, reinterpret_cast<hipStream_t>(stream));
}
