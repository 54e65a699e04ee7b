// lrf_mesh_texture.inl -- a texture atlas baked for an indexed triangle mesh from encoded frames (included by lrf_render.hip
// after lrf_mesh_raster.inl; it reuses to_camera and pts_finite_pos of lrf_points.inl and sm_face of lrf_mesh_smooth.inl; the
// wave-leader counts are lrf_compact.inl's, the host helpers lrf_host.inl's).  Per texel and frame: project, test visibility against the
// mesh's own rasterised depth, weight, sample, accumulate.  The state bytes are a fixed function of the frames in their order.
//
// 1. Layout: a fixed patch of P x P texels (4 <= P <= 64, K = P - 3) holds two faces; faces 2c and 2c + 1 share cell c of a grid
//    of rows x cols cells, rows = ceil(ceil(Nf / 2) / cols); the atlas is Ht = rows P by Wt = cols P, y down from the top.  Texel
//    (x, y): c = (y / P) cols + x / P, a = x % P, b = y % P; it belongs to face 2c when a + b <= P - 1, else to face 2c + 1 with
//    (a, b) <- (P - 1 - a, P - 1 - b).  Barycentric weights in fp32: beta = a / K, gamma = b / K, alpha = (1 - beta) - gamma.
//    Texels of a half outside the triangle take the face's plane extrapolated (alpha slightly negative): every texel of a half
//    is baked by one rule and a viewer's bilinear taps never leave the half.  A texel whose face index is >= Nf is empty.
// 2. pw_i = (alpha v0_i + beta v1_i) + gamma v2_i in fp32; n = (v1 - v0) x (v2 - v0) in fp64 from the fp32 corners, every
//    operation rounded on its own, nn = (nx nx + ny ny) + nz nz.  A face with an index outside [0, Nv) is never dereferenced;
//    it, a face with two equal indices, with a corner that is not finite or with nn == 0 receives nothing.
// 3. Per frame v in frame order: q = to_camera(M_v, pw), nz = -q.z, skipped unless nz > 0; u = q.x / nz f + cx - 0.5,
//    w = -q.y / nz f + cy - 0.5 (reproject's expressions), (iu, iw) = rint, ties to even, skipped outside the image.  Facing in
//    fp64: d = t_v - pw, s = (nx dx + ny dy) + nz dz, dd = (dx dx + dy dy) + dz dz; skipped when s <= 0 (unless two_sided) or
//    s s < (min_cos min_cos) (nn dd).  Visibility: dm = mesh_depth[v, iw, iu] finite and positive and |nz - dm| <= vis_tol dm in
//    fp32.  Weight wt = (float)((s s) / (nn (dd dd))): cos^2 over squared distance, no square root; skipped unless finite and
//    positive.  Colour: bilinear from frames [V,H,W,3] uint8, x0 = floorf(u), fx = u - x0, taps clamp(x0, 0, W - 1) and
//    clamp(x0 + 1, 0, W - 1), the same in y; per channel top = c00 + fx (c10 - c00), bot alike, c = top + fy (bot - top).
// 4. State: one float4 per texel [Ht,Wt,4] = (c_r, c_g, c_b, w), zero at creation.  blend 0 ("mean"): w += wt, c_k += wt c_k';
//    blend 1 ("best"): (c, w) replaced when wt > w, the earliest frame wins ties.  A lane walks the frames in the caller's
//    order: the same bytes however the frames are split over calls.
// 5. Resolve: mean c_k / w, best c_k; rintf (ties to even), clamp to [0, 255], uint8.  mask = 1 where w > 0.  An unobserved
//    texel of a face whose indices are in range takes, when the mesh has rgb8, its vertex colours under the weights clamped to
//    [0, 1] and renormalised, in fp64 as k_rs_resolve: rint((w0 c0 + w1 c1) + w2 c2); otherwise and for an empty texel: fill.
//    info (int64 [8]): faces with an index out of range, with two equal indices, with a corner not finite, with nn == 0 (each
//    counted by the texel at its corner 0); texels used (face < Nf), observed, coloured by the fallback, empty.
//
// Work distribution.  One lane per texel, cell-major: t = c P^2 + b P + a, so a wave's 64 texels touch at most a few faces.
// k_tx_bake loops the frames inside the kernel; the state is read once and written once per call as one 128-bit access.  Pose,
// focal and centre loads are wave-uniform.  Per frame a ballot of "some lane passes nz / image / facing" lets the wave skip
// the depth and colour gathers together.  No LDS, no atomics, no scratch; no lane waits on another and every loop is bounded by
// V.  k_tx_resolve is one pass over the state with wave-leader integer atomics for info, which k_ag_zero
// (lrf_mesh_raster.inl) clears first.
namespace lrf {

constexpr int TX_NT = 256;

struct TextureArgs {
  const float* vertices; const uint8_t* rgb8; const int* faces;
  const uint8_t* frames; const float* mesh_depth; const float* c2w; const float* focal; const float* center;
  int Nv, Nf, P, cols, n_tex;                                       // n_tex = rows cols P^2 < 2^31
  int V, H, W, blend, two_sided;
  float vis_tol, min_cos;
};

// texel t (cell-major) -> its face (>= Nf: empty), (a, b) inside the face's half, and the float4 index of its state
struct Texel { int f, a, b; size_t at; };
__device__ __forceinline__ Texel tx_texel(const TextureArgs& g, int t) {
  const int pp = g.P * g.P;
  const int c = t / pp, r = t - c * pp;
  int b = r / g.P, a = r - b * g.P;
  const int cy = c / g.cols, cx = c - cy * g.cols;
  Texel x;
  x.at = (size_t)(cy * g.P + b) * ((size_t)g.cols * g.P) + (size_t)(cx * g.P + a);
  const bool odd = a + b > g.P - 1;
  if (odd) { a = g.P - 1 - a; b = g.P - 1 - b; }
  x.f = min(2 * c + (odd ? 1 : 0), g.Nf);                           // c < 2^31 / 16
  x.a = a; x.b = b;
  return x;
}

__device__ __forceinline__ void tx_weights(const TextureArgs& g, const Texel& x, float& alpha, float& beta, float& gamma) {
#pragma clang fp contract(off)
  const float K = (float)(g.P - 3);
  beta = (float)x.a / K;
  gamma = (float)x.b / K;
  alpha = (1.0f - beta) - gamma;
}

// step 2 -> 0: corners p, normal n and nn are set; 1, 2, 3: sm_face's kinds and a corner not finite; 4: nn == 0
__device__ __forceinline__ int tx_face(const TextureArgs& g, int f, float (&p)[3][3], int (&idx)[3], double (&n)[3], double& nn) {
#pragma clang fp contract(off)
  const int kind = sm_face(g.faces, f, g.Nv, &idx[0], &idx[1], &idx[2]);
  if (kind == 1) return 1;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[k][c] = g.vertices[3 * (size_t)idx[k] + c];
      finite = finite && (__float_as_uint(p[k][c]) & 0x7FFFFFFFu) < 0x7F800000u;
    }
  if (kind) return kind;
  if (!finite) return 3;
  double e1[3], e2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    e1[c] = (double)p[1][c] - (double)p[0][c];
    e2[c] = (double)p[2][c] - (double)p[0][c];
  }
  n[0] = e1[1] * e2[2] - e1[2] * e2[1];
  n[1] = e1[2] * e2[0] - e1[0] * e2[2];
  n[2] = e1[0] * e2[1] - e1[1] * e2[0];
  nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  return nn == 0.0 ? 4 : 0;
}

__global__ __launch_bounds__(TX_NT) void k_tx_bake(TextureArgs g, float4* __restrict__ state) {
#pragma clang fp contract(off)
  const long long tl = (long long)blockIdx.x * TX_NT + threadIdx.x;
  if (tl >= g.n_tex) return;
  const Texel x = tx_texel(g, (int)tl);
  float p[3][3], pw[3] = {0.0f, 0.0f, 0.0f};
  int idx[3];
  double n[3] = {0.0, 0.0, 0.0}, nn = 0.0;
  const bool live = x.f < g.Nf && tx_face(g, x.f, p, idx, n, nn) == 0;
  if (!__ballot(live)) return;                                      // a wave of empty texels or skipped faces: nothing to read
  float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (live) {
    float alpha, beta, gamma;
    tx_weights(g, x, alpha, beta, gamma);
#pragma unroll
    for (int c = 0; c < 3; ++c) pw[c] = (alpha * p[0][c] + beta * p[1][c]) + gamma * p[2][c];
    acc = state[x.at];
  }
  const float fo = g.focal[0], cx = g.center[0], cy = g.center[1];
  const double mc = (double)g.min_cos, mc2 = mc * mc;
  const size_t hw = (size_t)g.H * g.W;
  for (int v = 0; v < g.V; ++v) {
    const float* M = g.c2w + (size_t)v * 12;
    float q[3], nz = 0.0f, u = 0.0f, w = 0.0f;
    int iu = 0, iw = 0;
    double s = 0.0, dd = 0.0;
    bool pass = live;
    if (pass) {
      to_camera(M, pw, q);
      nz = -q[2];
      pass = nz > 0.0f;
    }
    if (pass) {
      u = q[0] / nz * fo + cx - 0.5f;
      w = -q[1] / nz * fo + cy - 0.5f;
      const float ru = rintf(u), rw = rintf(w);
      pass = ru >= 0.0f && ru < 2147483648.0f && rw >= 0.0f && rw < 2147483648.0f;   // NaN fails
      if (pass) {
        iu = (int)ru; iw = (int)rw;
        pass = iu < g.W && iw < g.H;
      }
    }
    if (pass) {
      const double dx = (double)M[3] - (double)pw[0], dy = (double)M[7] - (double)pw[1], dz = (double)M[11] - (double)pw[2];
      s = (n[0] * dx + n[1] * dy) + n[2] * dz;
      dd = (dx * dx + dy * dy) + dz * dz;
      pass = (g.two_sided || s > 0.0) && !(s * s < mc2 * (nn * dd));
    }
    if (!__ballot(pass)) continue;                                  // the wave skips this frame's gathers together
    if (!pass) continue;
    const float dm = g.mesh_depth[(size_t)v * hw + (size_t)iw * g.W + iu];
    if (!(pts_finite_pos(dm) && fabsf(nz - dm) <= g.vis_tol * dm)) continue;
    const float wt = (float)((s * s) / (nn * (dd * dd)));
    if (!(pts_finite_pos(wt))) continue;
    const float xf = floorf(u), yf = floorf(w);
    const float fx = u - xf, fy = w - yf;
    const int x0i = (int)xf, y0i = (int)yf;                         // in [-1, W - 1] x [-1, H - 1]: rint(u) is inside the image
    const int xa = min(max(x0i, 0), g.W - 1), xb = min(max(x0i + 1, 0), g.W - 1);
    const int ya = min(max(y0i, 0), g.H - 1), yb = min(max(y0i + 1, 0), g.H - 1);
    const uint8_t* img = g.frames + 3 * (size_t)v * hw;
    const uint8_t* t00 = img + 3 * ((size_t)ya * g.W + xa);
    const uint8_t* t10 = img + 3 * ((size_t)ya * g.W + xb);
    const uint8_t* t01 = img + 3 * ((size_t)yb * g.W + xa);
    const uint8_t* t11 = img + 3 * ((size_t)yb * g.W + xb);
    float col[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float c00 = (float)t00[c], c10 = (float)t10[c], c01 = (float)t01[c], c11 = (float)t11[c];
      const float top = c00 + fx * (c10 - c00);
      const float bot = c01 + fx * (c11 - c01);
      col[c] = top + fy * (bot - top);
    }
    if (g.blend == 0) {
      acc.x += wt * col[0]; acc.y += wt * col[1]; acc.z += wt * col[2]; acc.w += wt;
    } else if (wt > acc.w) {
      acc = make_float4(col[0], col[1], col[2], wt);
    }
  }
  if (live) state[x.at] = acc;
}

__device__ __forceinline__ float tx_byte(float x) {                 // NaN -> 0
  return fminf(fmaxf(rintf(x), 0.0f), 255.0f);
}

// fill: r | g << 8 | b << 16
__global__ __launch_bounds__(TX_NT) void k_tx_resolve(TextureArgs g, const float4* __restrict__ state, unsigned fill,
                                                      uint8_t* __restrict__ atlas, uint8_t* __restrict__ mask,
                                                      unsigned long long* __restrict__ info) {
#pragma clang fp contract(off)
  const long long tl = (long long)blockIdx.x * TX_NT + threadIdx.x;
  const bool in = tl < g.n_tex;
  int kind = -1;
  bool used = false, observed = false, fallback = false, corner = false;
  if (in) {
    const Texel x = tx_texel(g, (int)tl);
    used = x.f < g.Nf;
    float out[3] = {(float)(fill & 255u), (float)((fill >> 8) & 255u), (float)((fill >> 16) & 255u)};
    if (used) {
      float p[3][3];
      int idx[3];
      double n[3], nn;
      kind = tx_face(g, x.f, p, idx, n, nn);
      corner = x.a == 0 && x.b == 0;
      const float4 acc = state[x.at];
      observed = acc.w > 0.0f;
      if (observed) {
        if (g.blend == 0) { out[0] = tx_byte(acc.x / acc.w); out[1] = tx_byte(acc.y / acc.w); out[2] = tx_byte(acc.z / acc.w); }
        else { out[0] = tx_byte(acc.x); out[1] = tx_byte(acc.y); out[2] = tx_byte(acc.z); }
      } else if (g.rgb8 && kind != 1) {
        fallback = true;
        float alpha, beta, gamma;
        tx_weights(g, x, alpha, beta, gamma);
        double w0 = fmin(fmax((double)alpha, 0.0), 1.0), w1 = fmin(fmax((double)beta, 0.0), 1.0),
               w2 = fmin(fmax((double)gamma, 0.0), 1.0);
        const double sum = (w0 + w1) + w2;
        w0 = w0 / sum; w1 = w1 / sum; w2 = w2 / sum;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double c0 = (double)g.rgb8[3 * (size_t)idx[0] + c], c1 = (double)g.rgb8[3 * (size_t)idx[1] + c],
                       c2 = (double)g.rgb8[3 * (size_t)idx[2] + c];
          const double m = rint((w0 * c0 + w1 * c1) + w2 * c2);
          out[c] = (float)(m < 0.0 ? 0.0 : (m > 255.0 ? 255.0 : m));
        }
      }
    }
    atlas[3 * x.at] = (uint8_t)out[0]; atlas[3 * x.at + 1] = (uint8_t)out[1]; atlas[3 * x.at + 2] = (uint8_t)out[2];
    mask[x.at] = observed ? 1 : 0;
  }
  wave_count(&info[0], corner && kind == 1);
  wave_count(&info[1], corner && kind == 2);
  wave_count(&info[2], corner && kind == 3);
  wave_count(&info[3], corner && kind == 4);
  wave_count(&info[4], used);
  wave_count(&info[5], observed);
  wave_count(&info[6], fallback);
  wave_count(&info[7], in && !used);
}

// cols <= 0: the default, ceil(sqrt(n_cells)) by exact integer arithmetic (1 for no cell) -> texels, or -1 when refused
static long long texture_texels(long long Nf, long long P, long long& cols, long long& rows) {
  if (Nf < 0 || Nf >= (1ll << 31) || P < 4 || P > 64 || cols >= (1ll << 31)) return -1;
  const long long cells = (Nf + 1) / 2;
  if (cols <= 0) {
    long long r = 1;
    while (r * r < cells) ++r;                                      // at most 2^15 steps
    cols = r;
  }
  rows = (cells + cols - 1) / cols;
  if (rows * P >= (1ll << 31) || cols * P >= (1ll << 31)) return -1;
  const long long n = rows * cols;                                  // < 2^31 + 2^31
  return n * P * P < (1ll << 31) ? n * P * P : -1;
}

static int texture_args(const char* who, const LrfMeshTexture* m, bool frames, TextureArgs& a) {
  if (!m) return refuse(who, "null argument");
  long long cols = m->cols, rows = 0;
  if (m->cols < 1) return refuse(who, "need cols >= 1");
  const long long n = texture_texels(m->Nf, m->patch, cols, rows);
  if (n < 0 || m->Nv < 0 || m->Nv >= (1ll << 31) || (m->Nf > 0 && m->Nv < 1))
    return refuse(who, "need 4 <= patch <= 64, 0 <= Nf, 0 <= Nv < 2^31, vertices for the faces and fewer than 2^31 texels");
  if (m->Nf > 0 && (!m->vertices || !m->faces)) return refuse(who, "null argument");
  if (m->blend < 0 || m->blend > 1) return refuse(who, "blend must be 0 (mean) or 1 (best)");
  if (misaligned(3, m->vertices, m->faces, m->mesh_depth, m->cam2world, m->focal, m->center))
    return refuse(who, "float and int32 arrays must be 4-byte aligned");
  memset(&a, 0, sizeof(a));
  a.vertices = m->vertices; a.rgb8 = m->rgb8; a.faces = m->faces;
  a.Nv = (int)m->Nv; a.Nf = (int)m->Nf; a.P = m->patch; a.cols = m->cols; a.n_tex = (int)n; a.blend = m->blend;
  if (!frames) return 0;
  if (m->V < 1 || m->H < 1 || m->W < 1 || (long long)m->V * m->H * m->W >= (1ll << 31))
    return refuse(who, "need V, H, W >= 1 and V H W < 2^31");
  if (!m->frames || !m->mesh_depth || !m->cam2world || !m->focal || !m->center) return refuse(who, "null argument");
  if (m->two_sided < 0 || m->two_sided > 1) return refuse(who, "two_sided must be 0 or 1");
  if (!(m->vis_tol >= 0.0f)) return refuse(who, "vis_tol must be >= 0");
  if (!(m->min_cos >= 0.0f && m->min_cos <= 1.0f)) return refuse(who, "min_cos must lie in [0, 1]");
  a.frames = m->frames; a.mesh_depth = m->mesh_depth; a.c2w = m->cam2world; a.focal = m->focal; a.center = m->center;
  a.V = m->V; a.H = m->H; a.W = m->W; a.two_sided = m->two_sided; a.vis_tol = m->vis_tol; a.min_cos = m->min_cos;
  return 0;
}

}  // namespace lrf

extern "C" size_t lrf_mesh_texture_state_bytes(int64_t Nf, int32_t patch, int32_t cols) {
  long long c = cols, r = 0;
  const long long n = lrf::texture_texels(Nf, patch, c, r);
  return n < 0 ? 0 : (size_t)n * 16;
}

extern "C" int lrf_mesh_texture_bake(const LrfMeshTexture* m, float* state, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_texture_bake";
  TextureArgs a;
  if (texture_args(who, m, true, a)) return 1;
  if (a.n_tex && !state) return refuse(who, "null argument");
  if (misaligned(15, state)) return refuse(who, "state must be 16-byte aligned");
  if (!a.n_tex) return 0;
  return launch(k_tx_bake, blocks_for(a.n_tex, TX_NT), TX_NT, reinterpret_cast<hipStream_t>(stream), a,
                reinterpret_cast<float4*>(state));
}

extern "C" int lrf_mesh_texture_resolve(const LrfMeshTexture* m, const float* state, const uint8_t* fill, uint8_t* atlas,
                                        uint8_t* mask, int64_t* info, void* stream) {
  using namespace lrf;
  const char* who = "lrf_mesh_texture_resolve";
  TextureArgs a;
  if (texture_args(who, m, false, a)) return 1;
  if (!fill || !info || (a.n_tex && (!state || !atlas || !mask))) return refuse(who, "null argument");
  if (misaligned(15, state)) return refuse(who, "state must be 16-byte aligned");
  if (misaligned(7, info)) return refuse(who, "info must be 8-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* inf = reinterpret_cast<unsigned long long*>(info);
  LRF_TRY(launch(k_ag_zero, 1, RS_NT, st, inf, 8));                 // lrf_mesh_raster.inl's: info = 0
  if (!a.n_tex) return 0;
  const unsigned packed = (unsigned)fill[0] | (unsigned)fill[1] << 8 | (unsigned)fill[2] << 16;
  return launch(k_tx_resolve, blocks_for(a.n_tex, TX_NT), TX_NT, st, a, reinterpret_cast<const float4*>(state), packed, atlas,
                mask, inf);
}
