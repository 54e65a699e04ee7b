// lrf_tsdf_blocks.inl -- a block-sparse TSDF volume: only the 8 x 8 x 8 blocks that some depth pixel's truncation band reaches
// are stored, fused and meshed (included by lrf_render.hip after lrf_mesh.inl, which states the fusion and the meshing rules
// and holds their code: tsdf_fuse_point, mesh_count_body, mesh_emit_body, mesh_carve.  This file adds what is its own: which blocks
// exist, where a lattice point is stored, and in which order the pool is walked).
//
// The virtual lattice has 8Bx x 8By x 8Bz points at origin + (ix, iy, iz) * voxel: the dense lattice of those dims.  Stored:
//   marks  uint8 [Bz,By,Bx]   1 once a pixel's band met the block (cumulative over touch calls), else 0
//   table  int32 [Bz,By,Bx]   -1, or the block's pool index
//   coords int32 [n,3]        (bx, by, bz) of pool block k, in pool order
//   tsdf   [n,8,8,8] (starts at 1), weight [n,8,8,8] (starts at 0), rgb [n,8,8,8,3] (nullable, starts at 0), x fastest
// No hash: a block's pool index is a fixed function of the frames and the call sequence.  Everything below is fp32 with
// contraction off, so that a numpy restatement matches bit for bit.
//
// k_blocks_touch: one lane per depth pixel (v, row, col), plain byte stores of the value 1, no atomics:
//   1. d = depth[v,row,col]; skipped unless finite, positive and d_min <= d <= d_max;
//   2. dir = pixel_dir (lrf_scene.inl; z = -1); da = max(d - trunc, 0), db = d + trunc; the world points a, b at those depths
//      (world_point, lrf_points.inl);
//   3. m = voxel + db / focal: the lattice points whose nearest pixel this is lie within half a pixel footprint of the centre
//      ray (db / focal bounds it), and one voxel of rounding slack;
//   4. per axis l = min(a, b) - m, h = max(a, b) + m (skipped unless l <= h: a NaN marks nothing);
//      first = max(floor((l - origin) / (8 voxel)), 0), last = min(floor((h - origin) / (8 voxel)), B - 1), IEEE division;
//      skipped unless first <= last on the three axes;
//   5. marks[z, y, x] = 1 for every block of the box.
// Assignment is an ordered scan over the table in block-linear (z, y, x) order, three launches, no spinning:
//   k_blocks_flag    per workgroup of 256 table entries the number of fresh blocks (marked, table < 0)
//   k_points_scan    one workgroup: exclusive bases per workgroup, the number of fresh blocks in count[0]
//   k_blocks_assign  fresh block -> table = n_blocks + base + fresh blocks before it in its workgroup, unless n_blocks +
//                    count[0] exceeds max_blocks: then the table stays as it was.  coords[k] is (re)written for every block whose
//                    index k lies below the coords capacity.  Blocks allocated earlier keep their index.
//   With max_blocks = n_blocks no fresh block could fit: a counting call, flag and scan only.  The host counts, grows coords and
//   the pools, and only then lets the table change.
// k_blocks_fuse: one workgroup of 512 lanes per pool block, a wave is the 8 x 8 slab of consecutive x, y at one z.  The
//   block's coordinates come from coords[blockIdx]; ix = 8 bx + lx and so on; the rest is tsdf_fuse_point, so an allocated point
//   ends with the bits the dense kernel gives the same lattice point over the same frames.
// Extraction: BlocksMeshArgs is the view of the pool points.  A neighbour inside the block is the pool point beside it, one
//   outside is fetched through the table; a lattice point in no block is -1.  Weight gating is always on (min_weight > 0), so a
//   cell with a corner in no block is not valid: a missing block can leave a hole but never creates or moves a face.
//   Order: vertices in pool order, then (z, y, x, edge) inside the block; faces in pool order of the cell's lowest corner,
//   then (z, y, x) inside the block, then (tetrahedron, triangle).  Both depend on the block list alone.
namespace lrf {

constexpr int BLK_PTS = 512;                                        // 8 x 8 x 8
constexpr int BLK_NT = 256;                                         // table entries per workgroup (pool points: MESH_NT)
constexpr long long BLK_MAX_BLOCKS = (1ll << 22) - 1;               // 512 n < 2^31

struct BlocksArgs {
  uint8_t* marks; int* table; int* coords; float* tsdf; float* weight; float* rgb;
  int Bx, By, Bz, n_blocks;
  long long nb;                                                     // Bx By Bz
  float ox, oy, oz, voxel, trunc;
};

__global__ __launch_bounds__(BLK_NT) void k_blocks_touch(BlocksArgs a, const float* __restrict__ depth,
                                                         const float* __restrict__ c2w, const float* __restrict__ focal,
                                                         const float* __restrict__ center, int H, int W, long long n_px,
                                                         float d_min, float d_max) {
#pragma clang fp contract(off)
  const long long pl = (long long)blockIdx.x * BLK_NT + threadIdx.x;
  if (pl >= n_px) return;
  const float d = depth[pl];
  if (!(pts_finite_pos(d) && d >= d_min && d <= d_max)) return;
  const int per = H * W;
  const int v = (int)(pl / per), pix = (int)(pl - (long long)v * per);
  const float f = focal[0];
  const PixDir p = pixel_dir(pix, W, H, 0, f, center[0], center[1]);
  const float da = fmaxf(d - a.trunc, 0.0f), db = d + a.trunc;
  float pa[3], pb[3];
  world_point(c2w + (size_t)v * 12, p, da, pa);
  world_point(c2w + (size_t)v * 12, p, db, pb);
  const float m = a.voxel + db / f;
  const float bs = 8.0f * a.voxel;
  const float o[3] = {a.ox, a.oy, a.oz};
  const int B[3] = {a.Bx, a.By, a.Bz};
  int lo[3], hi[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float l = fminf(pa[k], pb[k]) - m, h = fmaxf(pa[k], pb[k]) + m;
    if (!(l <= h)) return;
    const float fl = fmaxf(floorf((l - o[k]) / bs), 0.0f), fh = fminf(floorf((h - o[k]) / bs), (float)(B[k] - 1));
    if (!(fl <= fh)) return;
    lo[k] = (int)fl;                                                // 0 <= fl <= fh <= 2^28
    hi[k] = min((int)fh, B[k] - 1);                                 // (float)(B - 1) may round up
  }
  for (int z = lo[2]; z <= hi[2]; ++z)
    for (int y = lo[1]; y <= hi[1]; ++y)
      for (int x = lo[0]; x <= hi[0]; ++x) a.marks[((size_t)z * a.By + y) * a.Bx + x] = 1;
}

__device__ __forceinline__ bool blocks_fresh(const BlocksArgs& a, long long i) {
  return i < a.nb && a.marks[i] != 0 && a.table[i] < 0;
}

__global__ __launch_bounds__(BLK_NT) void k_blocks_flag(BlocksArgs a, unsigned* __restrict__ wg) {
  __shared__ unsigned part[BLK_NT / 64];
  const long long i = (long long)blockIdx.x * BLK_NT + threadIdx.x;
  unsigned tot;
  block_scan_excl<BLK_NT>(blocks_fresh(a, i) ? 1u : 0u, part, tot);
  if (threadIdx.x == 0) wg[blockIdx.x] = tot;
}

__global__ __launch_bounds__(BLK_NT) void k_blocks_assign(BlocksArgs a, const unsigned* __restrict__ wg,
                                                          const long long* __restrict__ count, long long max_blocks,
                                                          long long coords_cap) {
  __shared__ unsigned part[BLK_NT / 64];
  const long long i = (long long)blockIdx.x * BLK_NT + threadIdx.x;
  const bool fresh = blocks_fresh(a, i);
  unsigned tot;
  const unsigned pre = block_scan_excl<BLK_NT>(fresh ? 1u : 0u, part, tot);
  if (i >= a.nb) return;
  long long idx = a.table[i];
  if (fresh && a.n_blocks + count[0] <= max_blocks) {
    idx = (long long)a.n_blocks + wg[blockIdx.x] + pre;             // < max_blocks <= BLK_MAX_BLOCKS
    a.table[i] = (int)idx;
  }
  if (idx >= 0 && idx < coords_cap) {
    const long long r = i / a.Bx;
    a.coords[3 * idx] = (int)(i - r * a.Bx); a.coords[3 * idx + 1] = (int)(r % a.By); a.coords[3 * idx + 2] = (int)(r / a.By);
  }
}

__global__ __launch_bounds__(BLK_PTS) void k_blocks_fuse(BlocksArgs a, const float* __restrict__ depth,
                                                         const uint8_t* __restrict__ rgb8, const float* __restrict__ c2w,
                                                         const float* __restrict__ focal, const float* __restrict__ center, int V,
                                                         int H, int W, float d_min, float d_max) {
#pragma clang fp contract(off)
  const int b = blockIdx.x;
  const int ix = 8 * a.coords[3 * b] + (threadIdx.x & 7), iy = 8 * a.coords[3 * b + 1] + ((threadIdx.x >> 3) & 7),
            iz = 8 * a.coords[3 * b + 2] + (threadIdx.x >> 6);
  const float pw[3] = {a.ox + (float)ix * a.voxel, a.oy + (float)iy * a.voxel, a.oz + (float)iz * a.voxel};
  tsdf_fuse_point((size_t)b * BLK_PTS + threadIdx.x, pw, a.tsdf, a.weight, a.rgb, a.trunc, depth, rgb8, c2w, focal, center, V, H, W,
                  d_min, d_max);
}

// ------------------------------------------------------------------------------------------------ extraction
// the view of the pool points: storage index = 512 block + (lz 8 + ly) 8 + lx
struct BlocksMeshArgs {
  const int* table; const int* coords; const float* value; const float* weight; const float* rgb;   // rgb nullable
  int Bx, By, Bz, n;                                                // n = 512 n_blocks < 2^31
  float ox, oy, oz, voxel, level, min_weight;

  __device__ __forceinline__ MeshPoint point(int p) const {
    __builtin_assume(p >= 0);                                       // a stored point: its own reads need no guard
    const int b = p >> 9;
    return {p, 8 * coords[3 * b] + (p & 7), 8 * coords[3 * b + 1] + ((p >> 3) & 7), 8 * coords[3 * b + 2] + ((p >> 6) & 7)};
  }
  __device__ __forceinline__ int beside(const MeshPoint& q, int dx, int dy, int dz) const {
    const int nx = (q.p & 7) + dx, ny = ((q.p >> 3) & 7) + dy, nz = ((q.p >> 6) & 7) + dz;
    if (!((nx | ny | nz) & ~7)) return q.p + dx + 8 * dy + 64 * dz;   // inside the block
    const int gx = q.x + dx, gy = q.y + dy, gz = q.z + dz;            // 8 B < 2^31: no overflow
    if (gx < 0 || gy < 0 || gz < 0 || gx >= 8 * Bx || gy >= 8 * By || gz >= 8 * Bz) return -2;
    const int b = table[((size_t)(gz >> 3) * By + (gy >> 3)) * Bx + (gx >> 3)];
    if (b < 0 || b >= (n >> 9)) return -1;
    return b * BLK_PTS + ((gz & 7) << 6 | (gy & 7) << 3 | (gx & 7));
  }
  __device__ __forceinline__ int corner(const MeshPoint& q, int d) const { return beside(q, d & 1, (d >> 1) & 1, (d >> 2) & 1); }
  __device__ __forceinline__ bool stored(int o) const { return o >= 0; }
  __device__ __forceinline__ float val(int o) const { return o >= 0 ? value[o] : 1.0f; }
  __device__ __forceinline__ bool passes(int o) const { return o >= 0 && weight[o] >= min_weight; }
  __device__ __forceinline__ float colour(int o, int c) const { return o >= 0 ? rgb[3 * (size_t)o + c] : 0.0f; }
};

__global__ __launch_bounds__(MESH_NT) void k_blocks_count(BlocksMeshArgs a, unsigned* __restrict__ info, unsigned* __restrict__ wgv,
                                                          unsigned* __restrict__ wgf) {
  __shared__ unsigned part[MESH_NT / 64];
  mesh_count_body(a, part, info, wgv, wgf);
}

__global__ __launch_bounds__(MESH_NT) void k_blocks_emit(BlocksMeshArgs a, const unsigned* __restrict__ info,
                                                        const unsigned* __restrict__ wgv, const unsigned* __restrict__ wgf,
                                                        long long max_vertices, long long max_faces, float* __restrict__ vertices,
                                                        uint8_t* __restrict__ rgb8_out, int* __restrict__ faces) {
  __shared__ unsigned part[MESH_NT / 64];
  mesh_emit_body(a, part, info, wgv, wgf, max_vertices, max_faces, vertices, rgb8_out, faces);
}

// blocks of a grid, or 0 when the entry points refuse it: each of Bx, By, Bz >= 1, 8 B < 2^31, Bx By Bz < 2^31
static long long blocks_grid(int Bx, int By, int Bz) {
  if (Bx < 1 || By < 1 || Bz < 1 || Bx >= (1 << 28) || By >= (1 << 28) || Bz >= (1 << 28)) return 0;
  const long long n = (long long)Bx * By;                            // < 2^56
  return n >= (1ll << 31) || n * Bz >= (1ll << 31) ? 0 : n * Bz;
}

// the workspace of an assignment: the fresh blocks of each workgroup of BLK_NT table entries
static unsigned* blocks_assign_wg(Carver& c, long long nb) { return c.take<unsigned>(blocks_for(nb, BLK_NT)); }

// the checks the four entry points share; 0 when the volume passes
static int blocks_check(const char* who, const LrfTsdfBlocks* g, bool pools, BlocksArgs& a) {
  if (!g) return refuse(who, "null argument");
  const long long nb = blocks_grid(g->Bx, g->By, g->Bz);
  if (!nb) return refuse(who, "need Bx, By, Bz >= 1, 8 B < 2^31 per axis and Bx By Bz < 2^31");
  if (g->n_blocks < 0 || g->n_blocks > BLK_MAX_BLOCKS) return refuse(who, "need 0 <= n_blocks and 512 n_blocks < 2^31");
  if (!g->table || !g->coords || (pools ? !g->tsdf || !g->weight : !g->marks)) return refuse(who, "null argument");
  if (!(g->voxel > 0.0f)) return refuse(who, "voxel must be > 0");
  if (!(g->trunc > 0.0f)) return refuse(who, "trunc must be > 0");
  if (misaligned(3, g->table, g->coords, g->tsdf, g->weight, g->rgb)) return refuse(who, "float and int32 arrays must be 4-byte aligned");
  memset(&a, 0, sizeof(a));
  a.marks = g->marks; a.table = g->table; a.coords = g->coords; a.tsdf = g->tsdf; a.weight = g->weight; a.rgb = g->rgb;
  a.Bx = g->Bx; a.By = g->By; a.Bz = g->Bz; a.n_blocks = g->n_blocks; a.nb = nb;
  a.ox = g->origin[0]; a.oy = g->origin[1]; a.oz = g->origin[2]; a.voxel = g->voxel; a.trunc = g->trunc;
  return 0;
}

}  // namespace lrf

extern "C" int lrf_tsdf_blocks_touch(const LrfTsdfBlocks* g, const float* depth, const float* cam2world, const float* focal,
                                     const float* center, int32_t V, int32_t H, int32_t W, float d_min, float d_max,
                                     void* stream) {
  using namespace lrf;
  BlocksArgs a;
  if (blocks_check("lrf_tsdf_blocks_touch", g, false, a)) return 1;
  if (tsdf_check_frames("lrf_tsdf_blocks_touch", depth, cam2world, focal, center, V, H, W, d_min, d_max)) return 1;
  const long long n_px = (long long)V * H * W;
  return launch(k_blocks_touch, blocks_for(n_px, BLK_NT), BLK_NT, reinterpret_cast<hipStream_t>(stream), a, depth, cam2world, focal,
                center, H, W, n_px, d_min, d_max);
}

extern "C" size_t lrf_tsdf_blocks_assign_workspace_bytes(int32_t Bx, int32_t By, int32_t Bz) {
  using namespace lrf;
  const long long nb = blocks_grid(Bx, By, Bz);
  if (!nb) return 0;
  Carver c(nullptr);
  blocks_assign_wg(c, nb);
  return c.bytes();
}

extern "C" int lrf_tsdf_blocks_assign(const LrfTsdfBlocks* g, int64_t max_blocks, int64_t coords_capacity, int64_t* count,
                                      void* workspace, void* stream) {
  using namespace lrf;
  BlocksArgs a;
  if (blocks_check("lrf_tsdf_blocks_assign", g, false, a)) return 1;
  if (!count || !workspace) return set_err("lrf_tsdf_blocks_assign: null argument");
  if (max_blocks < 0 || max_blocks > BLK_MAX_BLOCKS) return set_err("lrf_tsdf_blocks_assign: need 0 <= max_blocks and 512 max_blocks < 2^31");
  if (coords_capacity < 0 || coords_capacity >= (1ll << 31))
    return set_err("lrf_tsdf_blocks_assign: coords_capacity must lie in [0, 2^31)");
  if (misaligned(3, workspace)) return set_err("lrf_tsdf_blocks_assign: float and int32 arrays must be 4-byte aligned");
  if (misaligned(7, count)) return set_err("lrf_tsdf_blocks_assign: count must be 8-byte aligned");
  const int n_wg = (int)blocks_for(a.nb, BLK_NT);
  Carver c(workspace);
  unsigned* wg = blocks_assign_wg(c, a.nb);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LRF_TRY(launch(k_blocks_flag, n_wg, BLK_NT, st, a, wg));
  LRF_TRY(launch(k_points_scan, 1, PTS_SCAN_NT, st, wg, n_wg, reinterpret_cast<long long*>(count)));
  if (max_blocks == a.n_blocks) return 0;                            // a counting call: no fresh block could fit
  return launch(k_blocks_assign, n_wg, BLK_NT, st, a, wg, reinterpret_cast<const long long*>(count), max_blocks, coords_capacity);
}

extern "C" int lrf_tsdf_blocks_integrate(const LrfTsdfBlocks* g, const float* depth, const uint8_t* rgb8, const float* cam2world,
                                         const float* focal, const float* center, int32_t V, int32_t H, int32_t W, float d_min,
                                         float d_max, void* stream) {
  using namespace lrf;
  BlocksArgs a;
  if (blocks_check("lrf_tsdf_blocks_integrate", g, true, a)) return 1;
  if (tsdf_check_frames("lrf_tsdf_blocks_integrate", depth, cam2world, focal, center, V, H, W, d_min, d_max)) return 1;
  if (!g->rgb != !rgb8) return set_err("lrf_tsdf_blocks_integrate: the volume's rgb and the frames' rgb8 go together");
  if (a.n_blocks == 0) return 0;                                     // no block: nothing to launch
  return launch(k_blocks_fuse, a.n_blocks, BLK_PTS, reinterpret_cast<hipStream_t>(stream), a, depth, rgb8, cam2world, focal, center,
                V, H, W, d_min, d_max);
}

extern "C" size_t lrf_mesh_extract_blocks_workspace_bytes(int32_t n_blocks) {
  using namespace lrf;
  if (n_blocks < 0 || n_blocks > BLK_MAX_BLOCKS) return 0;
  return mesh_carve(nullptr, (long long)n_blocks * BLK_PTS, 1).bytes;   // never 0 for an accepted count
}

extern "C" int lrf_mesh_extract_blocks(const LrfTsdfBlocks* g, float level, float min_weight, int64_t max_vertices,
                                       int64_t max_faces, float* vertices, uint8_t* rgb8_out, int32_t* faces, int64_t* counts,
                                       void* workspace, void* stream) {
  using namespace lrf;
  BlocksArgs b;
  if (blocks_check("lrf_mesh_extract_blocks", g, true, b)) return 1;
  if (mesh_check_outputs("lrf_mesh_extract_blocks", g->rgb != nullptr, level, true, min_weight, max_vertices, max_faces, vertices,
                         rgb8_out, faces, counts, workspace))
    return 1;
  BlocksMeshArgs a;
  memset(&a, 0, sizeof(a));
  a.table = b.table; a.coords = b.coords; a.value = b.tsdf; a.weight = b.weight; a.rgb = b.rgb;
  a.Bx = b.Bx; a.By = b.By; a.Bz = b.Bz; a.n = b.n_blocks * BLK_PTS;
  a.ox = b.ox; a.oy = b.oy; a.oz = b.oz; a.voxel = b.voxel; a.level = level; a.min_weight = min_weight;
  const MeshWs w = mesh_carve(workspace, a.n, 1);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (w.n_wg) LRF_TRY(launch(k_blocks_count, w.n_wg, MESH_NT, st, a, w.info, w.wgv, w.wgf));
  LRF_TRY(launch(k_points_scan, 2, PTS_SCAN_NT, st, w.wgv, w.n_wg, reinterpret_cast<long long*>(counts)));
  if (!w.n_wg || (max_vertices == 0 && max_faces == 0)) return 0;     // no block, or a counting call: no row could be written
  return launch(k_blocks_emit, w.n_wg, MESH_NT, st, a, w.info, w.wgv, w.wgf, max_vertices, max_faces, vertices, rgb8_out, faces);
}
