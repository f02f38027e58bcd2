// Part 3 canonical decoder on the fused 8x256 chain: NeRFDecoder on [code(x) | code(t)] (reference src/core.py:108-113 and
// 233-281, src/decoders.py:29-87) for `canonical_type: nerf` (code(x_c) L 10, code(t') L 10: 84 columns) and for
// `direct_time_conditioning` (code(x) L 10, code(t) L <= 10).  Plan: p3canon_plan.h.
//
//   fwd_kernel     mlp_chain_body.h::chain_forward, the body of the vanilla compiler-scheduled forward (mlp_fwd.hip), on this
//                  plan: six natural code k-steps at pts_layers.0 and at the skip; the codes are formed in registers from
//                  x [n,3] and t [n] (and formed again at the skip instead of being held live through layers 0..3).  TRAIN:
//                  blocked bf16 images of every layer input and the ReLU masks, as the vanilla forward writes them.
//   fwd_scalar_time_kernel   the inference forward at ONE time read from a device word (CanonCodeScalar), for the evaluation launch
//                  chain nerf_p3_nerf_render_rays_fwd (render_p3_nerf.hip); the same bits as fwd_kernel<false> at that time.
//   dgrad_kernel   mlp_chain_body.h::chain_dgrad, the body of mlp_bwd.hip::mlp_bwd_kernel, on this layout's dgrad stream:
//                  pre-activation gradient images.
//   dcode_kernel   d code(x) = W0[:, :63]^T dz0 + W4[:, 256:319]^T dz4 from the bf16 images of dz0 / dz4, then the Fourier
//                  chain rule to d x [n,3], ADDED to the caller's vector (x_c = x + delta_x).
//   weight grads   mlp_wgrad.hip's split-K kernel with this decoder's job table (partial tiles + ordered reduction into a
//                  gradient image of fixed layout), then remap_kernel into the reference layout.
#include <stddef.h>
#include <stdint.h>
#include "mlp_chain_body.h"
#include "mlp_stash.h"
#include "mlp_wgrad.h"
#include "p3canon_plan.h"

namespace nerf {
namespace p3c {
using plan::Step;

// ---------------------------------------------------------------------------------------------------- codes
// time code of one scalar, [t | sin(2^0 pi t) | cos(2^0 pi t) | sin(2^1 pi t) | ...] (src/embeddings.py:28-32, input_dim 1),
// always the L = 10 width (21 features; a narrower code is its prefix: the packer zeroes the weight columns past time_dim)
struct TimeSpec { float scale; float phase; int raw; };   // raw: 0 trig, 1 t itself, 3 zero
constexpr TimeSpec time_spec(int f) {
  if (f == 0) return {1.0f, 0.0f, 1};
  if (f >= cplan::kTimeMax) return {1.0f, 0.0f, 3};
  const int c = f - 1;
  return {(float)(1 << (c >> 1)), (c & 1) ? 0.25f : 0.0f, 0};
}
__device__ __forceinline__ float time_eval(const TimeSpec s, float t) {
  if (s.raw == 1) return t;
  if (s.raw == 3) return 0.0f;
  return sincos_rev(t, s.scale, s.phase);
}
// B fragments (natural k order) of the time code: feature f = 16 ks + 8 half + j
template <int KS>
__device__ __forceinline__ void time_operand(float t, int half, bf16x8 (&out)[KS]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const TimeSpec s0 = time_spec(16 * ks + j), s1 = time_spec(16 * ks + 8 + j);
      float v;
      if (s0.raw == 0 && s1.raw == 0) v = sincos_rev(t, half ? s1.scale : s0.scale, half ? s1.phase : s0.phase);
      else v = half ? time_eval(s1, t) : time_eval(s0, t);
      out[ks][j] = (__bf16)v;
    }
  }
}
// the six code k-steps of one sample: [code(x) 63 | 1 | code(t) 21 | 0 ...]
__device__ __forceinline__ void code_operand(float x0, float x1, float x2, float t, int half, bf16x8 (&code)[cplan::kCodeKs]) {
  bf16x8 xe[4], te[2];
  fourier_operand<4, cplan::kPosDim>(x0, x1, x2, half, xe);
  time_operand<2>(t, half, te);
#pragma unroll
  for (int i = 0; i < 4; ++i) code[i] = xe[i];
  code[4] = te[0];
  code[5] = te[1];
}

// ---------------------------------------------------------------------------------------------------- workspace
// split-K partial tiles of the weight gradients: one tile per (workgroup, job) of at most kTileFloats floats (the merged
// feature + sigma job: 256 x 256 + 256 + 257, rounded up to 64), at most min(kSlabMaxWorkgroups, wave tiles x jobs / 4)
// workgroups (wgrad_launch's grid) plus one extra tile per job.  Sized by n: small batches keep a small workspace and the
// partial-tile form (the same bits every run) at every size.  A device with more CUs than kSlabMaxWorkgroups makes
// wgrad_launch fall back to float atomics rather than overrun it.
constexpr int kWgradJobs = 12;
constexpr size_t kTileFloats = (256 * 256 + 256 + 257 + 63) / 64 * 64;
inline size_t slab_bytes(int64_t n) {
  const int64_t want = (n + kWaveSamples - 1) / kWaveSamples * kWgradJobs / 4;
  const int64_t grid = want < 1 ? 1 : (want > (int64_t)kSlabMaxWorkgroups ? (int64_t)kSlabMaxWorkgroups : want);
  return (size_t)(grid + kWgradJobs) * kTileFloats * sizeof(float);
}

struct Layout {
  int64_t n_pad;
  size_t xenc, h, feat, hv, denc, mask;             // forward images (bf16) and ReLU masks
  size_t dsmall, dhv, dfeat, dh;                     // dgrad images
  size_t egrad, slab, slab_bytes, total;             // weight-gradient image and the split-K partial tiles
};
inline Layout layout(int64_t n) {
  Layout s{};
  s.n_pad = (n + 255) / 256 * 256;
  const size_t np = (size_t)s.n_pad;
  size_t o = 0;
  s.xenc = take(&o, np * cplan::kCodeK * 2);
  s.h = take(&o, np * 256 * 2 * 8);
  s.feat = take(&o, np * 256 * 2);
  s.hv = take(&o, np * 128 * 2);
  s.denc = take(&o, np * 32 * 2);
  s.mask = take(&o, (np / 256) * 9 * 512 * 16);
  s.dsmall = take(&o, np * 16 * 2);
  s.dhv = take(&o, np * 128 * 2);
  s.dfeat = take(&o, np * 256 * 2);
  s.dh = take(&o, np * 256 * 2 * 8);
  s.egrad = take(&o, (size_t)cplan::eCount * 4);
  s.slab_bytes = slab_bytes(n);
  s.slab = take(&o, s.slab_bytes);
  s.total = o;
  return s;
}

// ---------------------------------------------------------------------------------------------------- forward
struct FwdArgs {
  const char* packed;
  const float* x;        // [n,3] position fed to code(x) (x_c, or x under direct time conditioning)
  const float* t;        // [n]
  const float* dirs;     // [n,3] view directions (encoded as given)
  int64_t n, n_pad;
  float* rgb;
  float* sigma;
  __bf16* st_xenc;       // nat [n_pad, 96]
  __bf16* st_h;          // 8 x blocked [n_pad, 256]
  __bf16* st_feat;
  __bf16* st_hv;
  __bf16* st_denc;       // nat [n_pad, 32]
  uint4* st_mask;        // [tiles][9][512]: word (m>>1), bits 16*(m&1) + r (the compiler-scheduled family's masks)
};

// mlp_chain_body.h::chain_forward on this plan.  The forward chain walks cplan's chunk table and runs mtile<KS> on a pointer
// (the generated asm m-tiles have no 6 or 22 k-step form).  The code operand keeps x and t, not the six operand registers:
// the skip layer forms the code again from them: the same arithmetic on the same values (the same bits), 20 VGPRs fewer
// live through layers 0..3.
struct CanonCode {
  static constexpr int kKs = cplan::kCodeKs;
  float x0, x1, x2, t;
  __device__ __forceinline__ void form(const FwdArgs& a, int64_t nc, int half, bf16x8 (&code)[kKs], bf16x8 (&denc)[2]) {
    x0 = a.x[nc * 3 + 0]; x1 = a.x[nc * 3 + 1]; x2 = a.x[nc * 3 + 2]; t = a.t[nc];
    code_operand(x0, x1, x2, t, half, code);
    fourier_operand<2, plan::kDirDim>(a.dirs[nc * 3 + 0], a.dirs[nc * 3 + 1], a.dirs[nc * 3 + 2], half, denc);
  }
  __device__ __forceinline__ void again(int half, const bf16x8 (&)[kKs], bf16x8 (&out)[kKs]) const {
    code_operand(x0, x1, x2, t, half, out);
  }
};
struct CanonFwd {
  using Chain = nerf::Chain<cplan::kFwdChunks, cplan::step_of, false, false>;
  using Code = CanonCode;
  static constexpr size_t kStreamOff = cplan::kPackFwdOff, kBiasOff = cplan::kPackBiasOff;
};

template <bool TRAIN>
__global__ void __launch_bounds__(kChainThreads, 2) fwd_kernel(const FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, half = lane >> 5;
  chain_forward<CanonFwd, TRAIN>(a, smem, tid, lane, wave, col, half);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last pass's look-ahead DMA must not outlive the wave
}

// The canonical chain of the Part 3 (8x256 canonical field) evaluation launch chain (nerf_p3_nerf_render_rays_fwd): fwd_kernel<false>
// at ONE time, read from DEVICE memory.  CanonCodeScalar is CanonCode with t = *a.time_dev instead of a.t[nc]: code_operand, the
// direction code and again() are the same calls on the same values, so rgb and sigma keep fwd_kernel<false>'s bits when a.t holds that
// time in every row.  The training-image pointers exist because chain_forward names them; TRAIN is false and they stay NULL.
struct FwdScalarArgs {
  const char* packed;
  const float* x;        // [n,3] x_c, or x under direct time conditioning
  const float* time_dev; // ONE fp32
  const float* dirs;     // [n,3]
  int64_t n, n_pad;
  float* rgb;
  float* sigma;
  __bf16* st_xenc;
  __bf16* st_h;
  __bf16* st_feat;
  __bf16* st_hv;
  __bf16* st_denc;
  uint4* st_mask;
};
struct CanonCodeScalar {
  static constexpr int kKs = cplan::kCodeKs;
  float x0, x1, x2, t;
  __device__ __forceinline__ void form(const FwdScalarArgs& a, int64_t nc, int half, bf16x8 (&code)[kKs], bf16x8 (&denc)[2]) {
    x0 = a.x[nc * 3 + 0]; x1 = a.x[nc * 3 + 1]; x2 = a.x[nc * 3 + 2]; t = *a.time_dev;
    code_operand(x0, x1, x2, t, half, code);
    fourier_operand<2, plan::kDirDim>(a.dirs[nc * 3 + 0], a.dirs[nc * 3 + 1], a.dirs[nc * 3 + 2], half, denc);
  }
  __device__ __forceinline__ void again(int half, const bf16x8 (&)[kKs], bf16x8 (&out)[kKs]) const {
    code_operand(x0, x1, x2, t, half, out);
  }
};
struct CanonFwdScalar {
  using Chain = nerf::Chain<cplan::kFwdChunks, cplan::step_of, false, false>;
  using Code = CanonCodeScalar;
  static constexpr size_t kStreamOff = cplan::kPackFwdOff, kBiasOff = cplan::kPackBiasOff;
};

__global__ void __launch_bounds__(kChainThreads, 2) fwd_scalar_time_kernel(const FwdScalarArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, half = lane >> 5;
  chain_forward<CanonFwdScalar, false>(a, smem, tid, lane, wave, col, half);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last pass's look-ahead DMA must not outlive the wave
}

// ---------------------------------------------------------------------------------------------------- dgrad
struct BwdArgs {
  const char* packed;
  const float* rgb;
  const float* sigma;
  const float* d_rgb;
  const float* d_sigma;
  int64_t n, n_pad;
  const uint4* st_mask;
  __bf16* dsmall;        // nat [n_pad,16]: cols 0..2 d(rgb_pre), col 3 d(sigma_pre)
  __bf16* dhv;           // blocked [n_pad,128]
  __bf16* dfeat;         // blocked [n_pad,256]
  __bf16* dh;            // 8 x blocked [n_pad,256]: dh[l] = d(pre-activation of pts_layers.l)
};

// mlp_chain_body.h::chain_dgrad on this layout's transposed stream (the vanilla steps and chunks: the code columns are never
// contracted)
__global__ void __launch_bounds__(kChainThreads, 2) dgrad_kernel(const BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, half = lane >> 5;
  chain_dgrad<cplan::kPackBwdOff>(a, smem, tid, lane, wave, col, half);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---------------------------------------------------------------------------------------------------- d x through the code
struct DcodeArgs {
  const char* packed;
  const char* dh0;       // blocked bf16 images of dz0, dz4 (dgrad_kernel)
  const char* dh4;
  const float* x;        // [n,3] the code's input
  int64_t n;
  float* d_x;            // [n,3] += d loss / d x
};

// One wave per 32-sample wave tile.  The image blocks ARE the accumulator-order B operands the dgrad chain consumed
// (stash_block); A = the d-code stream (code rows 0..63 of W0^T and W4[:, 256:]^T, rows 63 zero), straight from global
// memory (64 KiB, L2-resident).  Lane (c, h) ends with d code[row] of sample c for its 32 rows, row = 32 mt + (r&3) +
// 8 (r>>2) + 4 h; the chain rule of [x | sin(2^b pi x) | cos(2^b pi x)]: d sin = 2^b pi cos, d cos = -2^b pi sin, in
// revolutions sin(2 pi (r + 1/4)).
__global__ void __launch_bounds__(256) dcode_kernel(const DcodeArgs a) {
  const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
  const int64_t wave_tiles = (a.n + kWaveSamples - 1) / kWaveSamples;
  const char* A = a.packed + cplan::kPackGradOff + lane * 16;
  constexpr float kPiF = 3.14159265358979f;
  for (int64_t wt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); wt < wave_tiles; wt += (int64_t)gridDim.x * 4) {
    f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][r] = 0.0f;
#pragma unroll
    for (int part = 0; part < 2; ++part) {
      const char* img = (part ? a.dh4 : a.dh0) + wt * 8 * 2048 + block_lane_offset(col, half);
      bf16x8 b[16];
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        b[2 * m] = *reinterpret_cast<const bf16x8*>(img + m * 2048);
        b[2 * m + 1] = *reinterpret_cast<const bf16x8*>(img + m * 2048 + 128);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
          const bf16x8 af = *reinterpret_cast<const bf16x8*>(A + ((part * 2 + mt) * 16 + ks) * 1024);
          acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, b[ks], acc[mt], 0, 0, 0);
        }
    }
    const int64_t n = wt * kWaveSamples + col;
    const bool live = n < a.n;
    const int64_t nc = live ? n : a.n - 1;
    const float x0 = a.x[nc * 3 + 0], x1 = a.x[nc * 3 + 1], x2 = a.x[nc * 3 + 2];
    float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row0 = 32 * mt + (r & 3) + 8 * (r >> 2);
        const FeatSpec s0 = feat_spec<cplan::kPosDim>(row0), s1 = feat_spec<cplan::kPosDim>(row0 + 4);
        const int axis = half ? s1.axis : s0.axis, raw = half ? s1.raw : s0.raw;
        const float xa = axis == 0 ? x0 : (axis == 1 ? x1 : x2);
        float deriv = 0.0f;
        if (raw == 1) deriv = 1.0f;
        else if (raw == 0) {
          const float scale = half ? s1.scale : s0.scale, phase = half ? s1.phase : s0.phase;
          deriv = kPiF * scale * sincos_rev(xa, scale, phase + 0.25f);
        }
        const float g = acc[mt][r] * deriv;
        d0 += axis == 0 ? g : 0.0f;
        d1 += axis == 1 ? g : 0.0f;
        d2 += axis == 2 ? g : 0.0f;
      }
    d0 += __shfl_xor(d0, 32);
    d1 += __shfl_xor(d1, 32);
    d2 += __shfl_xor(d2, 32);
    if (live && half == 0) {
      a.d_x[n * 3 + 0] += d0;
      a.d_x[n * 3 + 1] += d1;
      a.d_x[n * 3 + 2] += d2;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- packing
// fragment descriptors: forward stream (cplan steps), dgrad stream (vanilla steps), d-code stream (kind kGrad + part)
constexpr int kGradKind = plan::kNumKinds;
constexpr int kAllFrags = cplan::kFwdFrags + cplan::kBwdFrags + cplan::kGradFrags;
struct FragTable { int v[kAllFrags]; };
constexpr FragTable make_frag_table() {
  FragTable t{};
  int f = 0;
  for (int kind = plan::F_PTS0; kind <= plan::F_RGB; ++kind)
    for (int m = 0; m < cplan::step_of(kind).mt; ++m)
      for (int k = 0; k < plan::step_ks(kind, cplan::step_of); ++k) t.v[f++] = (kind << 16) | (m << 8) | k;
  for (int kind = plan::B_RGB; kind <= plan::B_PTS1; ++kind)
    for (int m = 0; m < plan::step_of(kind).mt; ++m)
      for (int k = 0; k < plan::step_ks(kind); ++k) t.v[f++] = (kind << 16) | (m << 8) | k;
  for (int part = 0; part < 2; ++part)
    for (int m = 0; m < 2; ++m)
      for (int k = 0; k < 16; ++k) t.v[f++] = ((kGradKind + part) << 16) | (m << 8) | k;
  return t;
}
__constant__ FragTable g_frag_table = make_frag_table();

// flat parameter index feeding A[row][k] of a step, or -1 for structural zeros
__device__ __forceinline__ int src_index(const cplan::Layout& L, int td, int kind, int row, int k, bool nat) {
  using namespace plan;
  switch (kind) {
    case F_PTS0: {
      const int c = cplan::code_col(k, td);
      return c < 0 ? -1 : L.W0 + row * L.C + c;
    }
    case F_PTS4: {
      const int c = nat ? cplan::code_col(k, td) : k;
      return c < 0 ? -1 : L.W4 + row * (256 + L.C) + (nat ? 256 + c : c);
    }
    case F_PTS1: case F_PTS2: case F_PTS3: case F_PTS5: case F_PTS6: case F_PTS7:
      return L.weight_off(kind) + row * 256 + k;
    case F_HEAD: return row < 256 ? L.tail(kWFeat) + row * 256 + k : (row == 256 ? L.tail(kWSigma) + k : -1);
    case F_VIEW: return nat ? (k < 27 ? L.tail(kWView) + row * 283 + 256 + k : -1) : L.tail(kWView) + row * 283 + k;
    case F_RGB: return row < 3 ? L.tail(kWRgb) + row * 128 + k : -1;
    case B_RGB: return k < 3 ? L.tail(kWRgb) + k * 128 + row : -1;
    case B_VIEW: return L.tail(kWView) + k * 283 + row;
    case B_HEAD: return nat ? (k == 0 ? L.tail(kWSigma) + row : -1) : L.tail(kWFeat) + k * 256 + row;
    case kGradKind:       // d code: A[j][k] = W0[k][j]
      return row < cplan::kPosDim ? L.W0 + k * L.C + row : -1;
    case kGradKind + 1:   // A[j][k] = W4[k][256 + j]
      return row < cplan::kPosDim ? L.W4 + k * (256 + L.C) + 256 + row : -1;
    default: {
      const int l = 7 - (kind - B_PTS7);                  // B_PTS7..B_PTS1: transposed pts_layers.l
      return L.weight_off(l) + k * L.in_dim(l) + row;
    }
  }
}

__global__ void __launch_bounds__(256) pack_kernel(const float* __restrict__ params, int td, char* __restrict__ packed) {
  const cplan::Layout L = cplan::layout(td);
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < kAllFrags * 64; t += gridDim.x * blockDim.x) {
    const int frag = t >> 6, lane = t & 63;
    const int desc = g_frag_table.v[frag];
    const int kind = desc >> 16, mt = (desc >> 8) & 0xFF, ks = desc & 0xFF;
    const Step st = kind < plan::kNumKinds ? (kind <= plan::F_RGB ? cplan::step_of(kind) : plan::step_of(kind)) : Step{2, 16, 0};
    const int row = mt * 32 + (lane & 31), h = lane >> 5;
    const bool nat = ks >= st.ks_acc;
    bf16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = frag_column(nat ? ks - st.ks_acc : ks, h, j, nat);
      const int src = src_index(L, td, kind, row, k, nat);
      out[j] = (__bf16)(src >= 0 ? params[src] : 0.0f);
    }
    size_t off;
    if (frag < cplan::kFwdFrags) off = cplan::kPackFwdOff + (size_t)frag * 1024;
    else if (frag < cplan::kFwdFrags + cplan::kBwdFrags) off = cplan::kPackBwdOff + (size_t)(frag - cplan::kFwdFrags) * 1024;
    else off = cplan::kPackGradOff + (size_t)(frag - cplan::kFwdFrags - cplan::kBwdFrags) * 1024;
    *reinterpret_cast<bf16x8*>(packed + off + lane * 16) = out;
  }
  float* bias = reinterpret_cast<float*>(packed + cplan::kPackBiasOff);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < plan::kBiasFloats; i += gridDim.x * blockDim.x) {
    float b = 0.0f;
    if (i < 2048) b = params[L.bias_off(i >> 8) + (i & 255)];
    else if (i < 2048 + 288) { const int r = i - 2048; b = r < 256 ? params[L.tail(plan::kBFeat) + r] : (r == 256 ? params[L.tail(plan::kBSigma)] : 0.0f); }
    else if (i < 2048 + 288 + 128) b = params[L.tail(plan::kBView) + (i - 2048 - 288)];
    else { const int r = i - 2048 - 288 - 128; b = r < 3 ? params[L.tail(plan::kBRgb) + r] : 0.0f; }
    bias[i] = b;
  }
}

// gradient image (cplan::e*) -> reference layout, every parameter written once
__global__ void __launch_bounds__(256) remap_kernel(const float* __restrict__ eg, int td, float* __restrict__ grads) {
  const cplan::Layout L = cplan::layout(td);
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < L.count; p += gridDim.x * blockDim.x) {
    int s;
    if (p < L.B0) s = cplan::eW0 + (p / L.C) * cplan::kCodeK + cplan::code_k(p % L.C, td);
    else if (p < L.W1) s = cplan::eB0 + (p - L.B0);
    else if (p < L.W4) s = cplan::eW1 + (p - L.W1);
    else if (p < L.B4) {
      const int q = p - L.W4, o = q / (256 + L.C), c = q % (256 + L.C);
      s = c < 256 ? cplan::eW4h + o * 256 + c : cplan::eW4c + o * cplan::kCodeK + cplan::code_k(c - 256, td);
    } else if (p < L.W5) s = cplan::eB4 + (p - L.B4);
    else if (p < L.WSigma) s = cplan::eW5 + (p - L.W5);
    else s = cplan::eWSigma + (p - L.WSigma);
    grads[p] = eg[s];
  }
}

// split-K weight gradients (mlp_wgrad.hip) into the gradient image; jobs in the vanilla order
int launch_wgrad(const char* ws, const Layout& wl, int64_t n, hipStream_t stream) {
  using namespace cplan;
  WgradArgs args{};
  const size_t np = (size_t)wl.n_pad;
  const char* xenc = ws + wl.xenc;
  auto st_h = [&](int l) { return ws + wl.h + (size_t)l * np * 256 * 2; };
  auto dh = [&](int l) { return ws + wl.dh + (size_t)l * np * 256 * 2; };
  int nj = 0;
  {  // pts_layers.0: dz0 x code (96 columns in k order; bias from the constant column 63)
    WgradJob j{};
    j.a = dh(0); j.a_bytes = 16384; j.mt_a = 8;
    j.b_nat = xenc; j.b_nat_bytes = 1024 * kCodeKs; j.nt_nat = 3;
    j.w_off = eW0; j.w_ld = kCodeK; j.o_valid = 256; j.nat_valid = kCodeK; j.nat_col0 = 0;
    j.bias_off = eB0; j.bias_nat_col = 63; j.kind = 14;
    args.jobs[nj++] = j;
  }
  for (int l = 1; l < 8; ++l) {
    WgradJob j{};
    j.a = dh(l); j.a_bytes = 16384; j.mt_a = 8;
    j.b_acc = st_h(l - 1); j.b_acc_bytes = 16384; j.nt_acc = 8; j.ones = 1; j.bias_nat_col = -1;
    j.w_ld = 256; j.o_valid = 256; j.acc_valid = 256; j.kind = 0;
    if (l == 4) {          // hidden columns here, the code columns in the next job (11 column tiles exceed kMaxTiles)
      j.w_off = eW4h; j.bias_off = eB4;
    } else {
      j.w_off = e_weight_off(l); j.bias_off = e_weight_off(l) + 256 * 256;
    }
    args.jobs[nj++] = j;
    if (l == 4) {          // pts_layers.4, code columns: dz4 x code
      WgradJob c{};
      c.a = dh(4); c.a_bytes = 16384; c.mt_a = 8;
      c.b_nat = xenc; c.b_nat_bytes = 1024 * kCodeKs; c.nt_nat = 3;
      c.w_off = eW4c; c.w_ld = kCodeK; c.o_valid = 256; c.nat_valid = kCodeK; c.nat_col0 = 0; c.bias_nat_col = -1; c.kind = 14;
      args.jobs[nj++] = c;
    }
  }
  {  // feature_layer + sigma_layer on the stream of h7
    WgradJob j{};
    j.a = ws + wl.dfeat; j.a_bytes = 16384; j.mt_a = 8;
    j.b_acc = st_h(7); j.b_acc_bytes = 16384; j.nt_acc = 8; j.ones = 1; j.bias_nat_col = -1;
    j.w_off = e_tail(plan::kWFeat); j.w_ld = 256; j.o_valid = 256; j.acc_valid = 256; j.bias_off = e_tail(plan::kBFeat);
    j.a2 = ws + wl.dsmall; j.w2_off = e_tail(plan::kWSigma); j.bias2_off = e_tail(plan::kBSigma); j.o2_row = 3; j.n2 = 257; j.kind = 13;
    args.jobs[nj++] = j;
  }
  {  // view_layer: dHv x [feat | denc]
    WgradJob j{};
    j.a = ws + wl.dhv; j.a_bytes = 8192; j.mt_a = 4;
    j.b_acc = ws + wl.feat; j.b_acc_bytes = 16384; j.nt_acc = 8;
    j.b_nat = ws + wl.denc; j.b_nat_bytes = 2048; j.nt_nat = 1; j.nat_valid = 27; j.nat_col0 = 256; j.bias_nat_col = 27;
    j.w_off = e_tail(plan::kWView); j.w_ld = 283; j.o_valid = 128; j.acc_valid = 256; j.bias_off = e_tail(plan::kBView); j.kind = 3;
    args.jobs[nj++] = j;
  }
  {  // rgb_layer: dsmall[:,0:3] x hv
    WgradJob j{};
    j.a = ws + wl.dsmall; j.a_bytes = 1024; j.a_nat = 1; j.mt_a = 1; j.split_n = 1;
    j.b_acc = ws + wl.hv; j.b_acc_bytes = 8192; j.nt_acc = 4; j.ones = 1; j.bias_nat_col = -1;
    j.w_off = e_tail(plan::kWRgb); j.w_ld = 128; j.o_row0 = 0; j.o_valid = 3; j.acc_valid = 128; j.bias_off = e_tail(plan::kBRgb); j.kind = 5;
    args.jobs[nj++] = j;
  }
  args.n_jobs = nj;
  if (nj != kWgradJobs) return fail(NERF_EINVAL, "nerf_p3_canon_bwd: %d weight-gradient jobs, the workspace is sized for %d", nj, kWgradJobs);
  float* eg = reinterpret_cast<float*>(const_cast<char*>(ws) + wl.egrad);
  float* slab = reinterpret_cast<float*>(const_cast<char*>(ws) + wl.slab);
  // partial tiles and an ordered sum: the same bits every run (a launch too small for contiguous spans falls back to atomics
  // on a zeroed image)
  return wgrad_launch(args, n, eg, stream, slab, wl.slab_bytes, 0, (size_t)cplan::eCount);
}

}  // namespace p3c
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_p3_canon_param_count(int time_dim) {
  return time_dim >= 1 && time_dim <= cplan::kTimeMax ? cplan::layout(time_dim).count : -1;
}
extern "C" size_t nerf_p3_canon_packed_bytes(void) { return cplan::kPackBytes; }
extern "C" size_t nerf_p3_canon_workspace_bytes(int64_t n) { return n > 0 ? p3c::layout(n).total : 0; }

extern "C" int nerf_p3_canon_pack(const float* params_f32, int time_dim, void* packed, nerf_stream_t stream) {
  NERF_REQUIRE(params_f32 && packed && ((uintptr_t)packed & 255) == 0, "nerf_p3_canon_pack: bad pointer");
  NERF_REQUIRE(time_dim >= 1 && time_dim <= cplan::kTimeMax, "nerf_p3_canon_pack: time_dim=%d (1..%d)", time_dim, cplan::kTimeMax);
  hipLaunchKernelGGL(p3c::pack_kernel, dim3(512), dim3(256), 0, as_stream(stream), params_f32, time_dim, static_cast<char*>(packed));
  return check_launch("nerf_p3_canon_pack");
}

extern "C" int nerf_p3_canon_fwd(const void* packed, void* workspace, const float* x, const float* t, const float* dirs, int64_t n,
                                 float* rgb, float* sigma, int train, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "nerf_p3_canon_fwd: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && x && t && dirs && rgb && sigma && ((uintptr_t)packed & 255) == 0, "nerf_p3_canon_fwd: bad pointer");
  NERF_REQUIRE(!train || (workspace && ((uintptr_t)workspace & 255) == 0), "nerf_p3_canon_fwd: training needs an aligned workspace");
  p3c::FwdArgs a{};
  const p3c::Layout l = p3c::layout(n);
  a.packed = static_cast<const char*>(packed);
  a.x = x; a.t = t; a.dirs = dirs; a.n = n; a.n_pad = l.n_pad; a.rgb = rgb; a.sigma = sigma;
  if (train) {
    char* w = static_cast<char*>(workspace);
    a.st_xenc = reinterpret_cast<__bf16*>(w + l.xenc);
    a.st_h = reinterpret_cast<__bf16*>(w + l.h);
    a.st_feat = reinterpret_cast<__bf16*>(w + l.feat);
    a.st_hv = reinterpret_cast<__bf16*>(w + l.hv);
    a.st_denc = reinterpret_cast<__bf16*>(w + l.denc);
    a.st_mask = reinterpret_cast<uint4*>(w + l.mask);
  }
  const int grid = grid_for(l.n_pad / kTileSamples, 1);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p3_canon_fwd: cannot query device");
  const void* kernel = train ? (const void*)p3c::fwd_kernel<true> : (const void*)p3c::fwd_kernel<false>;
  if (int rc = ensure_dynamic_lds(kernel, kChainLds, "nerf_p3_canon_fwd"); rc != NERF_OK) return rc;
  if (train) hipLaunchKernelGGL(p3c::fwd_kernel<true>, dim3(grid), dim3(kChainThreads), kChainLds, as_stream(stream), a);
  else hipLaunchKernelGGL(p3c::fwd_kernel<false>, dim3(grid), dim3(kChainThreads), kChainLds, as_stream(stream), a);
  return check_launch("nerf_p3_canon_fwd");
}

// The canonical launch of nerf_p3_nerf_render_rays_fwd per chunk (common.h; render_p3_nerf.hip has checked the entry's arguments): rows
// [0, n) of x / dirs at the time *time_dev, nerf_p3_canon_fwd's inference launch shape.
int nerf::p3_canon_fwd_scalar_time(const void* packed, const float* x, const float* dirs, int64_t n, const float* time_dev, float* rgb,
                                   float* sigma, nerf_stream_t stream) {
  NERF_REQUIRE(n > 0 && n < ((int64_t)1 << 31) && packed && x && dirs && time_dev && rgb && sigma && ((uintptr_t)packed & 255) == 0,
               "nerf_p3_nerf_render_rays_fwd (canonical chain): bad arguments");
  p3c::FwdScalarArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.x = x; a.time_dev = time_dev; a.dirs = dirs; a.n = n; a.n_pad = (n + 255) / 256 * 256; a.rgb = rgb; a.sigma = sigma;
  const int grid = grid_for(a.n_pad / kTileSamples, 1);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p3_nerf_render_rays_fwd: cannot query device");
  if (int rc = ensure_dynamic_lds((const void*)p3c::fwd_scalar_time_kernel, kChainLds, "nerf_p3_nerf_render_rays_fwd"); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(p3c::fwd_scalar_time_kernel, dim3(grid), dim3(kChainThreads), kChainLds, as_stream(stream), a);
  return check_launch("nerf_p3_nerf_render_rays_fwd (canonical chain)");
}

extern "C" int nerf_p3_canon_bwd(const void* packed, void* workspace, const float* x, const float* rgb, const float* sigma,
                                 const float* d_rgb, const float* d_sigma, int64_t n, int time_dim, float* grads_f32, float* d_x,
                                 nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "nerf_p3_canon_bwd: n=%lld", (long long)n);
  NERF_REQUIRE(time_dim >= 1 && time_dim <= cplan::kTimeMax, "nerf_p3_canon_bwd: time_dim=%d (1..%d)", time_dim, cplan::kTimeMax);
  NERF_REQUIRE(grads_f32 != nullptr, "nerf_p3_canon_bwd: grads_f32 is NULL");
  if (n == 0) {
    if (hipMemsetAsync(grads_f32, 0, sizeof(float) * cplan::layout(time_dim).count, as_stream(stream)) != hipSuccess)
      return fail(NERF_ELAUNCH, "nerf_p3_canon_bwd: memset failed");
    return NERF_OK;
  }
  NERF_REQUIRE(packed && workspace && rgb && sigma && d_rgb && d_sigma && ((uintptr_t)workspace & 255) == 0,
               "nerf_p3_canon_bwd: bad pointer");
  NERF_REQUIRE(d_x == nullptr || x != nullptr, "nerf_p3_canon_bwd: d_x needs x");
  const p3c::Layout l = p3c::layout(n);
  char* w = static_cast<char*>(workspace);
  p3c::BwdArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.rgb = rgb; a.sigma = sigma; a.d_rgb = d_rgb; a.d_sigma = d_sigma;
  a.n = n; a.n_pad = l.n_pad;
  a.st_mask = reinterpret_cast<const uint4*>(w + l.mask);
  a.dsmall = reinterpret_cast<__bf16*>(w + l.dsmall);
  a.dhv = reinterpret_cast<__bf16*>(w + l.dhv);
  a.dfeat = reinterpret_cast<__bf16*>(w + l.dfeat);
  a.dh = reinterpret_cast<__bf16*>(w + l.dh);
  const int grid = grid_for(l.n_pad / kTileSamples, 1);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p3_canon_bwd: cannot query device");
  if (int rc = ensure_dynamic_lds((const void*)p3c::dgrad_kernel, kChainLds, "nerf_p3_canon_bwd"); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(p3c::dgrad_kernel, dim3(grid), dim3(kChainThreads), kChainLds, as_stream(stream), a);
  if (int rc = check_launch("nerf_p3_canon_bwd (dgrad)"); rc != NERF_OK) return rc;
  if (d_x != nullptr) {
    p3c::DcodeArgs c{};
    c.packed = a.packed;
    c.dh0 = w + l.dh;
    c.dh4 = w + l.dh + (size_t)4 * l.n_pad * 256 * 2;
    c.x = x; c.n = n; c.d_x = d_x;
    const int64_t waves = (n + kWaveSamples - 1) / kWaveSamples, want = (waves + 3) / 4;
    hipLaunchKernelGGL(p3c::dcode_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, as_stream(stream), c);
    if (int rc = check_launch("nerf_p3_canon_bwd (d x)"); rc != NERF_OK) return rc;
  }
  if (int rc = p3c::launch_wgrad(w, l, n, as_stream(stream)); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(p3c::remap_kernel, dim3(1024), dim3(256), 0, as_stream(stream), reinterpret_cast<const float*>(w + l.egrad),
                     time_dim, grads_f32);
  return check_launch("nerf_p3_canon_bwd (remap)");
}
