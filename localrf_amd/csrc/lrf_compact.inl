// lrf_compact.inl -- what the scene-end geometry files (lrf_points.inl, lrf_mesh*.inl, lrf_tsdf_blocks.inl) share: the ordered
// compaction's scans and keep-list rank, the wave-leader atomics, k_points_scan and the small predicates in_range, is_finite
// and mesh_shape (included by lrf_render.hip ahead of lrf_points.inl).  Nothing here has fewer than two call sites.  The host
// helpers of the entry points (refuse, launch, misaligned, blocks_for, round_up, Carver) live in lrf_host.inl.
//
// Ordered compaction, as every one of those files does it: a mark pass leaves one keep bit per item (64-bit words) and a count
// per group of items, k_points_scan turns the group counts into exclusive bases, and a write pass sends a kept item to row
// base of its group + kept items before it in the group.  No atomics order the rows, so the output is the same on every run.
namespace lrf {

constexpr int PTS_SCAN_NT = 1024;
constexpr int KEEP_GROUP = 16;                                      // keep words per scanned group

__device__ __forceinline__ bool in_range(int i, int n) { return (unsigned)i < (unsigned)n; }
__host__ __device__ __forceinline__ bool is_finite(double x) { return x - x == 0.0; }

// inclusive prefix of v over each run of WIDTH lanes (every lane calls)
template <int WIDTH = 64>
__device__ __forceinline__ unsigned wave_scan_incl(unsigned v) {
  const int lane = threadIdx.x & (WIDTH - 1);
#pragma unroll
  for (int off = 1; off < WIDTH; off <<= 1) {
    const unsigned t = __shfl_up(v, off, WIDTH);
    if (lane >= off) v += t;
  }
  return v;
}

// exclusive prefix of v over the workgroup's NT threads (every thread calls), total = the workgroup's sum; part: NT / 64 words
// of LDS, free again on return
template <int NT>
__device__ __forceinline__ unsigned block_scan_excl(unsigned v, unsigned* part, unsigned& total) {
  static_assert(NT % 64 == 0 && NT <= 1024, "whole waves, one workgroup");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned s = wave_scan_incl(v);
  if (lane == 63) part[wv] = s;
  __syncthreads();
  unsigned pre = 0;
  total = 0;
  for (int w = 0; w < NT / 64; ++w) {
    const unsigned q = part[w];
    if (w < wv) pre += q;
    total += q;
  }
  __syncthreads();
  return pre + (s - v);
}

// a keep list: bit i of bits says item i is kept, pre[w] counts the kept items before word w inside its group of KEEP_GROUP
// words, wg[g] (after its scan) those before group g
struct KeepList {
  const unsigned long long* bits; const unsigned* pre; const unsigned* wg;

  // list `which` of a stack: bits, pre [n][words], wg [n][words / KEEP_GROUP]
  __device__ __forceinline__ KeepList pick(int which, size_t words) const {
    return {bits + which * words, pre + which * words, wg + which * (words / KEEP_GROUP)};
  }
  template <class I>
  __device__ __forceinline__ bool kept(I i) const { return (bits[i >> 6] >> (i & 63)) & 1ull; }
  // the kept items before item i: the row of a kept item
  template <class I>
  __device__ __forceinline__ unsigned rank(I i) const {
    const I w = i >> 6;
    return wg[w / KEEP_GROUP] + pre[w] + (unsigned)__popcll(bits[w] & ((1ull << (i & 63)) - 1ull));
  }
};

// every lane of the wave calls; one atomic per wave: *word |= bits if any lane says so ...
template <class T>
__device__ __forceinline__ void wave_or(T* word, bool pred, T bits) {
  const unsigned long long m = __ballot(pred);
  if ((threadIdx.x & 63) == 0 && m) atomicOr(word, bits);
}
// ... *word += the number of lanes that say so
__device__ __forceinline__ void wave_count(unsigned long long* word, bool pred) {
  const unsigned long long m = __ballot(pred);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(word, (unsigned long long)__popcll(m));
}

// one workgroup per array: workgroup b turns wg[b n_wg + i] into the sum of wg[b n_wg + 0..i) (modulo 2^32) and leaves the
// true total in count[b].  ONE workgroup walks an array rather than decoupled look-back: there is one uint32 per group (14 400
// for the points of 64 frames of 360 x 640), the scan is a fixed sequence with no spinning on other workgroups' progress, it is
// capturable and it cannot deadlock under any scheduling.
__global__ __launch_bounds__(PTS_SCAN_NT) void k_points_scan(unsigned* __restrict__ wg, int n_wg, long long* __restrict__ count) {
  __shared__ unsigned part[PTS_SCAN_NT / 64];
  wg += (size_t)blockIdx.x * n_wg;
  unsigned long long carry = 0;
  for (int base = 0; base < n_wg; base += PTS_SCAN_NT) {
    const int i = base + threadIdx.x;
    unsigned tot;
    const unsigned pre = block_scan_excl<PTS_SCAN_NT>(i < n_wg ? wg[i] : 0u, part, tot);
    if (i < n_wg) wg[i] = (unsigned)carry + pre;
    carry += tot;
  }
  if (threadIdx.x == 0) count[blockIdx.x] = (long long)carry;
}

static bool mesh_shape(long long Nv, long long Nf) { return Nv >= 1 && Nf >= 0 && Nv < (1ll << 31) && Nf < (1ll << 31); }

}  // namespace lrf
