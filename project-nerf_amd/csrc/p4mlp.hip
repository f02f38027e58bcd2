// Part 4 dual-hash dynamic field: the small networks of reference src/core.py:282-352 as fused
// bf16-MFMA register chains, replacing tinycudann FullyFusedMLP (HashDeformationDecoder, src/decoders.py:264-318;
// InstantNeRFDecoder at pos_dim 32 + 21, src/decoders.py:136-162 with src/core.py:222) and the nn.Linear
// TimeModulationNetwork (src/decoders.py:321-371).  PARITY of the tcnn internals UNPINNED (library absent); the
// checker is the reference's own Part 4 code around the stand-in tinycudann (golden g14).
//
//   deformation chain (one kernel per direction), per sample:
//     tcode = Fourier_10(t')                                   [t | sin | cos ...] 21 columns  (src/embeddings.py:28-32)
//     tm    = sigmoid(W_T2 relu(W_T1 tcode + b_T1) + b_T2)     time modulation, 64                 (decoders.py:368-371)
//     df    = sum_k w_k(t') feat_k,  w = normalised triangle weights around t = 0, .5, 1       (core.py:313-332)
//     dx    = scale * W_D3 relu(W_D2 relu(W_D1 [df | tm]))     bias-free 88 -> 64 -> 64 -> 3     (decoders.py:313-316)
//     x_c   = x + dx                                                                             (core.py:341)
//   canonical chain: InstantNeRFDecoder on [hash(x_c) (32) | tcode (21)] and the direction code  (core.py:344-349)
//
// The resident-weight register chain of resident_chain.h (step runner, LDS prologue, epilogues, pack loop); the canonical
// chain's two kernel bodies are imlp.hip's (instant_chain_body.h) under this file's policy.  The FORWARD chains contract fp16
// operands (v_mfma_f32_32x32x16_f16, what tinycudann's FullyFusedMLP computes in): delta_x moves x_canonical inside a
// hash grid whose finest cells are 4e-4 wide, and bf16's 8 mantissa bits put ~1e-3 of rounding on a displacement of
// 0.2 -- several cells; fp16 keeps it below one.  The backward chains and the training images stay bf16 (gradients span
// more binades than fp16 holds without a loss scale): every layer input is stashed as a blocked bf16 image for the
// shared split-K weight-gradient kernel (mlp_wgrad.hip).
//
// Parameter vector (fp32, [out,in] row-major; the layouts of the module's state dict, concatenated):
//   T1W [64,21] T1b [64] T2W [64,64] T2b [64]              time_modulation.net.{0,2}.{weight,bias}
//   D1 [64,96] D2 [64,64] D3 [16,64]                        deform_decoder.deform_net.params (cols: 24 hash | 64 tm | 8 pad)
//   S1 [64,64] S2 [16,64]                                   decoder.sigma_net.params       (cols: 32 hash | 21 tcode | pad)
//   C1 [64,48] C2 [64,64] C3 [16,64]                        decoder.color_net.params
//   scale [1]                                               deform_decoder.displacement_scale
#include "instant_chain_body.h"
#include "lattice.h"
#include "mlp_wgrad.h"

namespace nerf {
namespace p4 {
using namespace resident;

constexpr int kT1W = 0, kT1b = 1344, kT2W = 1408, kT2b = 5504, kD1 = 5568, kD2 = 11712, kD3 = 15808;
constexpr int kS1 = 16832, kS2 = 20928, kC1 = 21952, kC2 = 25024, kC3 = 29120, kScale = 30144, kParams = 30145;
constexpr int kTimeDim = 21, kHashDeform = 24, kDirDim = 27;
constexpr int kThreads = 256, kTile = 128;
static_assert(kThreads == kInstantThreads && kTile == kInstantTile, "the canonical chain runs instant_chain_body.h's geometry");

enum { T1, T2, D1, D2, D3, D3t, D2t, D1tT, D1tH, T2t, S1, S2, C1, C2, C3, C3t, C2t, C1t, S2t, S1t, kSteps };
constexpr Step step_of(int s) {
  switch (s) {
    case T1: return {2, 0, 2, 0};      // tcode (32 nat) -> 64
    case T2: return {2, 4, 0, 4};      // 64 -> 64
    case D1: return {2, 4, 2, 12};     // [tm (64) | df (32 nat)] -> 64
    case D2: return {2, 4, 0, 24};
    case D3: return {1, 4, 0, 32};     // 64 -> 3
    case D3t: return {2, 0, 1, 36};    // d(dx raw) (16 nat) -> d(hd2)
    case D2t: return {2, 4, 0, 38};
    case D1tT: return {2, 4, 0, 46};   // -> d(tm)
    case D1tH: return {1, 4, 0, 54};   // -> d(df)
    case T2t: return {2, 4, 0, 58};    // d(tm_pre) -> d(ht1)
    case S1: return {2, 0, 4, 66};     // [hash (32) | tcode (32)] nat -> 64
    case S2: return {1, 4, 0, 74};     // 64 -> 16
    case C1: return {2, 1, 2, 78};     // [h16 | dir code (32 nat)] -> 64
    case C2: return {2, 4, 0, 84};
    case C3: return {1, 4, 0, 92};
    case C3t: return {2, 0, 1, 96};
    case C2t: return {2, 4, 0, 98};
    case C1t: return {1, 4, 0, 106};   // h16 rows only
    case S2t: return {2, 1, 0, 110};
    default: return {1, 4, 0, 112};    // S1t: hash rows only
  }
}
constexpr int kFrags = 116;
constexpr int kDeformFwd0 = 0, kDeformFwdN = 36, kDeformBwd0 = 36, kDeformBwdN = 30;
constexpr int kCanonFwd0 = 66, kCanonFwdN = 30, kCanonBwd0 = 96, kCanonBwdN = 20;
constexpr size_t kPackBytes = (size_t)kFrags * 1024 + 256;   // + T2 bias table (64 fp32)
constexpr size_t kPackBiasOff = (size_t)kFrags * 1024;

// parameter index of weight (row, k) of a step, or -1 (zero padding); nat: k is a natural-order column
__device__ __forceinline__ int src_of(int step, int row, int k, bool nat) {
  switch (step) {
    case T1: return k < kTimeDim ? kT1W + row * 21 + k : (k == kTimeDim ? kT1b + row : -1);   // column 21 of the code is the constant 1
    case T2: return kT2W + row * 64 + k;
    case D1: return nat ? (k < kHashDeform ? kD1 + row * 96 + k : -1) : kD1 + row * 96 + kHashDeform + k;
    case D2: return kD2 + row * 64 + k;
    case D3: return row < 3 ? kD3 + row * 64 + k : -1;
    case D3t: return k < 3 ? kD3 + k * 64 + row : -1;
    case D2t: return kD2 + k * 64 + row;
    case D1tT: return kD1 + k * 96 + kHashDeform + row;
    case D1tH: return row < kHashDeform ? kD1 + k * 96 + row : -1;
    case T2t: return kT2W + k * 64 + row;
    case S1: return k < 32 + kTimeDim ? kS1 + row * 64 + k : -1;
    case S2: return row < 16 ? kS2 + row * 64 + k : -1;
    case C1: return nat ? (k < kDirDim ? kC1 + row * 48 + 16 + k : -1) : (k < 16 ? kC1 + row * 48 + k : -1);
    case C2: return kC2 + row * 64 + k;
    case C3: return row < 3 ? kC3 + row * 64 + k : -1;
    case C3t: return k < 3 ? kC3 + k * 64 + row : -1;
    case C2t: return kC2 + k * 64 + row;
    case C1t: return row < 16 ? kC1 + k * 48 + row : -1;
    case S2t: return k < 16 ? kS2 + k * 64 + row : -1;
    default: return row < 32 ? kS1 + k * 64 + row : -1;
  }
}

__global__ void __launch_bounds__(256) pack_kernel(const float* __restrict__ params, char* __restrict__ packed) {
  // forward chains: fp16 fragments; backward: bf16
  pack_fragments(params, packed, kFrags, kSteps, step_of, src_of, [](int step) { return step <= D3 || (step >= S1 && step <= C3); },
                 blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  if (blockIdx.x == 0 && threadIdx.x < 64) reinterpret_cast<float*>(packed + kPackBiasOff)[threadIdx.x] = params[kT2b + threadIdx.x];
}

// 1-D Fourier code of the time stamp, element f of [t | sin(2^0 pi t) | cos(2^0 pi t) | sin(2^1 pi t) | ...] (21 columns);
// ONE: column 21 = 1 (bias column of the time-modulation layer), else 0.  v[ks][j] = column 16 ks + 8 half + j.
template <int KS, bool ONE>
__device__ __forceinline__ void time_values(float t, int half, float (&v)[KS][8]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f = 16 * ks + 8 * half + j;                          // this lane's column: one sin/cos evaluation
      const int c = f > 0 ? f - 1 : 0;
      const float trig = sincos_rev(t, (float)(1u << (c >> 1)), (c & 1) ? 0.25f : 0.0f);
      v[ks][j] = f == 0 ? t : (f < kTimeDim ? trig : ((ONE && f == kTimeDim) ? 1.0f : 0.0f));
    }
  }
}
// Fourier code of a unit direction (src/embeddings.py:28-32, L = 4: 27 columns, zero pad), as fourier_operand computes it
template <int KS>
__device__ __forceinline__ void dir_values(float x0, float x1, float x2, int half, float (&v)[KS][8]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const FeatSpec s0 = feat_spec<kDirDim>(16 * ks + j), s1 = feat_spec<kDirDim>(16 * ks + 8 + j);
      const float v0 = s0.raw == 3 || s0.raw == 2 ? 0.0f : feat_eval<kDirDim>(s0, x0, x1, x2);
      const float v1 = s1.raw == 3 || s1.raw == 2 ? 0.0f : feat_eval<kDirDim>(s1, x0, x1, x2);
      v[ks][j] = half ? v1 : v0;
    }
  }
}
template <int KS>
__device__ __forceinline__ void cast_values(const float (&v)[KS][8], f16x8 (&h)[KS], bf16x8 (&b)[KS]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int j = 0; j < 8; ++j) { h[ks][j] = (_Float16)v[ks][j]; b[ks][j] = (__bf16)v[ks][j]; }
}

struct DeformArgs {
  const char* packed;
  const __bf16* feat[3];   // nat images [n_pad,32] of the three deformation grids at x', FP16 (features 0..23 valid)
  const float* t;          // [n] per-sample time stamp t' (after the optional noise)
  const float* blend;      // [n,3] explicit grid weights or NULL: triangle weights of t' (core.py:324-332)
  const float* x;          // [n,3] sample positions (x_c = x + dx)
  const float* params;     // flat fp32 parameters (displacement_scale is read from here)
  int64_t n, n_pad;
  float* dx;               // [n,3]
  float* xc;               // [n,3]
  float* raw;              // [n,3] dx / scale (training)
  // training stash
  __bf16* tc; __bf16* ht1; __bf16* tm; __bf16* df; __bf16* hd1; __bf16* hd2;
  uint4* mask;             // [tiles][256]: T1, D1, D2 relu bits
  float* wts;              // [n_pad,4] the blend weights used (training)
  // backward
  const float* d_dx;       // [n,3]
  __bf16* dzt1; __bf16* dzt2; __bf16* dzd1; __bf16* dzd2; __bf16* dsmall;
  float* d_feat[3];        // [n,24] fp32 gradients for the three grids' scatter
  float* g_scale;          // parameter-gradient slot of displacement_scale (accumulated)
  unsigned* sum_ws;        // non-null (option "deterministic"): workspace of common.h::ordered_block_sum for g_scale
  unsigned* amax_bits;     // non-null: kAmaxSlots words that max-accumulate the largest |d_feat| as fp32 bits (common.h; the hash scatter's scale)
  float2* grad_lm;         // non-null: INSTEAD of d_feat, level-major gradients [3 * 12][n] (virtual level = grid * 12 + level): the
                           // layout the binned hash scatter reads coalesced (its count pass writes it otherwise)
};

__device__ __forceinline__ void triangle_weights(float t, float (&w)[3]) {
  // clamp(1 - |t - a| / 0.5, 0, 1) around a = 0, 0.5, 1, normalised with + 1e-8 (reference src/core.py:324-332)
  const float a[3] = {0.0f, 0.5f, 1.0f};
  float s = 1e-8f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w[k] = fminf(fmaxf(1.0f - fabsf(t - a[k]) / 0.5f, 0.0f), 1.0f);
    s += w[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = w[k] / s;
}

template <bool TRAIN>
__global__ void __launch_bounds__(kThreads) deform_fwd_kernel(const DeformArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = resident_weights<kThreads>(smem, a.packed, kDeformFwd0, kDeformFwdN, tid, lane);
  float* bias_lds = reinterpret_cast<float*>(smem + kDeformFwdN * 1024);
  if (tid < 64) bias_lds[tid] = reinterpret_cast<const float*>(a.packed + kPackBiasOff)[tid];
  __syncthreads();
  const float scale = a.params[kScale];
  const int64_t n_tiles = a.n_pad / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t wt = tile * 4 + wave, n = wt * 32 + col;
    const bool live = n < a.n;
    const int64_t nc = live ? n : a.n - 1;
    const float t = a.t[nc];
    f16x8 tc[2];
    bf16x8 tc_b[2];
    {
      float v[2][8];
      time_values<2, true>(t, half, v);
      cast_values<2>(v, tc, tc_b);
    }
    uint32_t mw[3] = {0, 0, 0};
    // ---- time modulation (decoders.py:368-371) ----
    f16x8 ht1[4], tm[4];
    run_step<step_of, T1, 2>(wbase, tc, nullptr, Mfma16{}, relu_epilogue<TRAIN>(ht1, a.ht1, mw[0], wt, col, half));
    run_step<step_of, T2, 4>(wbase, ht1, nullptr, Mfma16{}, [&](auto mc, f32x16 acc) {
      constexpr int m = decltype(mc)::value;
      const f32x16 b = bias_tile(bias_lds, 32 * m, half);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 1.0f / (1.0f + __expf(-(acc[r] + b[r])));
      acc_to_operand16(acc, tm[2 * m], tm[2 * m + 1]);
      if constexpr (TRAIN) stash_tile(a.tm, wt, 2, m, col, half, acc, tm[2 * m], tm[2 * m + 1]);
    });
    // ---- tri-grid blend (core.py:313-336) ----
    float w[3];
    if (a.blend != nullptr) { w[0] = a.blend[nc * 3 + 0]; w[1] = a.blend[nc * 3 + 1]; w[2] = a.blend[nc * 3 + 2]; }
    else triangle_weights(t, w);
    f16x8 df[2];
    bf16x8 df_b[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const f16x8 f0 = load_nat<f16x8>(a.feat[0], wt, 2, ks, col, half), f1 = load_nat<f16x8>(a.feat[1], wt, 2, ks, col, half),
                  f2 = load_nat<f16x8>(a.feat[2], wt, 2, ks, col, half);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool valid = 16 * ks + 8 * half + j < kHashDeform;      // the hash forward leaves features 24..31 unwritten
        const float v = valid ? w[0] * (float)f0[j] + w[1] * (float)f1[j] + w[2] * (float)f2[j] : 0.0f;
        df[ks][j] = (_Float16)v;
        df_b[ks][j] = (__bf16)v;
      }
    }
    if constexpr (TRAIN) {
      stash_nat(a.tc, wt, 2, 0, col, half, tc_b[0]);
      stash_nat(a.tc, wt, 2, 1, col, half, tc_b[1]);
      stash_nat(a.df, wt, 2, 0, col, half, df_b[0]);
      stash_nat(a.df, wt, 2, 1, col, half, df_b[1]);
      if (half == 0) *reinterpret_cast<f32x4*>(a.wts + n * 4) = f32x4{w[0], w[1], w[2], 0.0f};
    }
    // ---- displacement decoder (decoders.py:313-316) ----
    f16x8 hd1[4], hd2[4];
    {
      f16x8 cat[6] = {tm[0], tm[1], tm[2], tm[3], df[0], df[1]};
      run_step<step_of, D1, 6>(wbase, cat, nullptr, Mfma16{}, relu_epilogue<TRAIN>(hd1, a.hd1, mw[1], wt, col, half));
    }
    run_step<step_of, D2, 4>(wbase, hd1, nullptr, Mfma16{}, relu_epilogue<TRAIN>(hd2, a.hd2, mw[2], wt, col, half));
    run_step<step_of, D3, 4>(wbase, hd2, nullptr, Mfma16{}, [&](auto, f32x16 acc) {
      if (live && half == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float d = acc[c] * scale;
          a.dx[n * 3 + c] = d;
          a.xc[n * 3 + c] = a.x[n * 3 + c] + d;
          if constexpr (TRAIN) a.raw[n * 3 + c] = acc[c];
        }
      }
    });
    if constexpr (TRAIN) a.mask[tile * kThreads + tid] = make_uint4(mw[0], mw[1], mw[2], 0);
  }
}

// The deformation chain of the occupancy-grid refresh (nerf_p4_grid_update): deform_fwd_kernel<false> for the cells of a lattice slab
// at ONE time stamp t, which is a time anchor (0, 0.5 or 1), storing x_c alone.  What that fixes, and why the bits stay the loop's:
//   * t is uniform, so the time code and the whole T1 -> T2 block are the same in every MFMA column of every tile (a column's
//     output depends on its own column's inputs only): computed ONCE per wave, before the tile loop, with the A fragments and the
//     T2 bias read from the packed image in global memory.  Only D1, D2, D3 (24 of the forward's 36 fragments) are resident in LDS.
//   * at an anchor triangle_weights gives exactly (1,0,0), (0,1,0) or (0,0,1) (the normaliser 1e-8f + 1 is 1.0f), so the blend
//     w0 f0 + w1 f1 + w2 f2 of FINITE features is the anchor grid's feature in value: the kernel reads that ONE image.  The loop's
//     sum may carry the other sign on an exact zero (0 * f of either sign is added); a zero of either sign in a B operand adds a
//     zero product to D1's accumulators, which start at +0 and therefore never hold -0 (a sum of zeros is -0 only if every term is),
//     so hd1 and everything behind it are unchanged.  Non-finite table entries would break this (0 * inf); they are not supported.
//   * x is lattice_node of the cell index (the value nerf_grid_lattice stores), x_c = fma(dx_raw, scale, x): the contraction the
//     compiler applies to deform_fwd_kernel's `x + acc * scale`, written out so that it does not depend on what else is stored.
struct DeformLatticeArgs {
  const char* packed;
  const __bf16* feat;      // nat image [n_pad,32] of the anchor's deformation grid at the slab's cells, FP16 (features 0..23 valid)
  const float* params;     // flat fp32 parameters (displacement_scale is read from here)
  float t;                 // the anchor
  int64_t cell0, n, n_pad; // first cell of the slab, its cells, rounded up to whole tiles
  int res;
  float bound, step;       // the lattice (lattice.h)
  float* xc;               // [n,3]
};
constexpr int kDeformLattice0 = step_of(D1).frag0, kDeformLatticeN = kDeformFwd0 + kDeformFwdN - kDeformLattice0;
static_assert(step_of(T1).frag0 == kDeformFwd0 && kDeformLattice0 == 12 && kDeformLatticeN == 24, "T1, T2 lead the forward fragment stream");

__global__ void __launch_bounds__(kThreads) deform_lattice_kernel(const DeformLatticeArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = resident_weights<kThreads>(smem, a.packed, kDeformLattice0, kDeformLatticeN, tid, lane);
  // ---- time modulation (decoders.py:368-371), once per wave: fragments and bias straight from the packed image ----
  f16x8 tm[4];
  {
    const char* gbase = a.packed + lane * 16;
    const float* bias = reinterpret_cast<const float*>(a.packed + kPackBiasOff);
    f16x8 tc[2], ht1[4];
    bf16x8 tc_b[2];
    float v[2][8];
    time_values<2, true>(a.t, half, v);
    cast_values<2>(v, tc, tc_b);
    uint32_t mw = 0;
    run_step<step_of, T1, 2>(gbase, tc, nullptr, Mfma16{}, relu_epilogue<false>(ht1, (__bf16*)nullptr, mw, 0, col, half));
    run_step<step_of, T2, 4>(gbase, ht1, nullptr, Mfma16{}, [&](auto mc, f32x16 acc) {
      constexpr int m = decltype(mc)::value;
      const f32x16 b = bias_tile(bias, 32 * m, half);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 1.0f / (1.0f + __expf(-(acc[r] + b[r])));
      acc_to_operand16(acc, tm[2 * m], tm[2 * m + 1]);
    });
  }
  __syncthreads();
  const float scale = a.params[kScale];
  const int64_t n_tiles = a.n_pad / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t wt = tile * 4 + wave, n = wt * 32 + col;
    const bool live = n < a.n;
    // ---- the anchor grid's features (core.py:313-336 with unit weights) ----
    f16x8 df[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const f16x8 f = load_nat<f16x8>(a.feat, wt, 2, ks, col, half);
#pragma unroll
      for (int j = 0; j < 8; ++j) df[ks][j] = 16 * ks + 8 * half + j < kHashDeform ? f[j] : (_Float16)0.0f;   // features 24..31 are unwritten
    }
    // ---- displacement decoder (decoders.py:313-316) ----
    uint32_t mw[2] = {0, 0};
    f16x8 hd1[4], hd2[4];
    {
      f16x8 cat[6] = {tm[0], tm[1], tm[2], tm[3], df[0], df[1]};
      run_step<step_of, D1, 6>(wbase, cat, nullptr, Mfma16{}, relu_epilogue<false>(hd1, (__bf16*)nullptr, mw[0], wt, col, half));
    }
    run_step<step_of, D2, 4>(wbase, hd1, nullptr, Mfma16{}, relu_epilogue<false>(hd2, (__bf16*)nullptr, mw[1], wt, col, half));
    run_step<step_of, D3, 4>(wbase, hd2, nullptr, Mfma16{}, [&](auto, f32x16 acc) {
      if (live && half == 0) {
        int i[3];
        lattice_cell(a.cell0 + n, a.res, i[0], i[1], i[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) a.xc[n * 3 + c] = __builtin_fmaf(acc[c], scale, lattice_node(i[c], a.res, a.bound, a.step));
      }
    });
  }
}

__global__ void __launch_bounds__(kThreads) deform_bwd_kernel(const DeformArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = resident_weights<kThreads>(smem, a.packed, kDeformBwd0, kDeformBwdN, tid, lane);
  __syncthreads();
  const float scale = a.params[kScale];
  float gscale_local = 0.0f, amax = 0.0f;
  const int64_t n_tiles = a.n_pad / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t wt = tile * 4 + wave, n = wt * 32 + col;
    const bool live = n < a.n;
    float g[3] = {0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float d = a.d_dx[n * 3 + c];
        g[c] = d * scale;                                           // dx = raw * scale
        if (half == 0) gscale_local += d * a.raw[n * 3 + c];
      }
    }
    const bf16x8 small = small_operand(g[0], g[1], g[2], half);
    stash_nat(a.dsmall, wt, 1, 0, col, half, small);
    const uint4 mask = a.mask[tile * kThreads + tid];
    bf16x8 gd2[4], gd1[4], gt2[4], gt1[4];
    { bf16x8 in[1] = {small}; run_step<step_of, D3t, 1>(wbase, in, nullptr, MfmaBf{}, grad_epilogue(gd2, a.dzd2, mask.z, wt, col, half)); }
    run_step<step_of, D2t, 4>(wbase, gd2, nullptr, MfmaBf{}, grad_epilogue(gd1, a.dzd1, mask.y, wt, col, half));
    // d(tm) -> through the sigmoid: d(tm_pre) = d(tm) tm (1 - tm), with the stashed (bf16) gate values
    run_step<step_of, D1tT, 4>(wbase, gd1, nullptr, MfmaBf{}, [&](auto mc, f32x16 acc) {
      constexpr int m = decltype(mc)::value;
      bf16x8 lo, hi;
      load_block(a.tm, wt, 2, m, col, half, lo, hi);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float s = (float)(r < 8 ? lo[r] : hi[r - 8]);
        acc[r] *= s * (1.0f - s);
      }
      acc_to_operand(acc, gt2[2 * m], gt2[2 * m + 1]);
      stash_block(a.dzt2, wt, 2, m, col, half, gt2[2 * m], gt2[2 * m + 1]);
    });
    // d(df) -> the three grids, each weighted by its blend weight
    run_step<step_of, D1tH, 4>(wbase, gd1, nullptr, MfmaBf{}, [&](auto, f32x16 acc) {
      if (live) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(a.wts + n * 4);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
          for (int q = 0; q < 3; ++q) {                              // rows 8q + 4 half + (0..3) < 24
            f32x4 v = {acc[4 * q] * w[k], acc[4 * q + 1] * w[k], acc[4 * q + 2] * w[k], acc[4 * q + 3] * w[k]};
            if (a.grad_lm != nullptr) {                              // levels 4q + 2 half, + 1 of grid k
              float2* lm = a.grad_lm + (int64_t)(k * (kHashDeform / 2) + 4 * q + 2 * half) * a.n + n;
              lm[0] = make_float2(v[0], v[1]);
              lm[a.n] = make_float2(v[2], v[3]);
            } else *reinterpret_cast<f32x4*>(a.d_feat[k] + n * kHashDeform + 8 * q + 4 * half) = v;
          }
        }
        if (a.amax_bits != nullptr) {             // the largest STORED gradient (the scale the counting form would find)
          float m = 0.0f;
#pragma unroll
          for (int r = 0; r < 12; ++r) m = fmaxf(m, fabsf(acc[r]));
          amax = fmaxf(amax, m * fmaxf(fmaxf(w[0], w[1]), w[2]));
        }
      }
    });
    run_step<step_of, T2t, 4>(wbase, gt2, nullptr, MfmaBf{}, grad_epilogue(gt1, a.dzt1, mask.x, wt, col, half));
    (void)gt1;
  }
  // one atomic per workgroup (same-address float atomics retire one after the other in L2)
  __shared__ float gscale_part[kThreads / 64];
  gscale_local = wave_sum(gscale_local);
  if (lane == 0) gscale_part[threadIdx.x >> 6] = gscale_local;
  __syncthreads();
  float sum = 0.0f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) sum += gscale_part[w];
  }
  if (a.sum_ws != nullptr) {               // option "deterministic": the workgroups' sums added in workgroup order
    const float val[1] = {sum};
    float* const out[1] = {a.g_scale};
    ordered_block_sum<1>(val, out, a.sum_ws);
  } else if (threadIdx.x == 0 && sum != 0.0f) atomicAdd(a.g_scale, sum);
  if (a.amax_bits != nullptr) publish_amax_slots(amax, a.amax_bits);
}

// ------------------------------------------------------------------------------------------------ canonical chain
struct CanonArgs {
  const char* packed;
  const __bf16* hash_nat;  // nat [n_pad,32] FP16 from nerf_hash_encode_fwd_nat (nat_dtype 1) at x_c
  const float* t;          // [n]
  const float* dirs;       // [n,3] unit view directions
  int64_t n, n_pad;
  float* rgb; float* sigma;
  __bf16* sin_nat;         // training: [n_pad,64] nat image [hash | tcode] (the sigma-net's input, wgrad operand)
  __bf16* hs1; __bf16* h16; __bf16* denc; __bf16* hc1; __bf16* hc2;
  uint4* mask;
  const float* d_rgb; const float* d_sigma;
  __bf16* dzs1; __bf16* dzs2; __bf16* dzc1; __bf16* dzc2; __bf16* dsmall;
  float* d_feat;           // [n,32]
  unsigned* amax_bits;     // non-null: kAmaxSlots words that max-accumulate the largest |d_feat| as fp32 bits (common.h; the hash scatter's scale)
  float2* grad_lm;         // non-null: INSTEAD of d_feat, level-major gradients [16][n]
};

// what instant_chain_body.h needs to know of this decoder: fp16 forward operands with bf16 images of the same values, four natural
// k-steps [hash (32) | tcode (21, zero pad)] into the sigma-net, gradients accumulated by the caller (nothing cleared here)
struct CanonPolicy {
  static constexpr StepFn step_of = p4::step_of;
  static constexpr int S1 = p4::S1, S2 = p4::S2, C1 = p4::C1, C2 = p4::C2, C3 = p4::C3;
  static constexpr int C3t = p4::C3t, C2t = p4::C2t, C1t = p4::C1t, S2t = p4::S2t, S1t = p4::S1t;
  static constexpr int kFwd0 = kCanonFwd0, kFwdN = kCanonFwdN, kBwd0 = kCanonBwd0, kBwdN = kCanonBwdN;
  static constexpr int kSigmaKs = 4;
  static constexpr bool kZeroGrads = false, kFence = false;
  using V = f16x8;
  using Mfma = Mfma16;
  // the sigma-net's input alone at ONE time stamp (instant_sigma): the two k-steps of the hash operand image and the time code of
  // the scalar a.t -- what operands<false> forms for sin[0..3]
  template <class A>
  static __device__ __forceinline__ void sigma_operands(const A& a, int64_t wt, int col, int half, f16x8 (&sin)[4]) {
    sin[0] = load_nat<f16x8>(a.hash_nat, wt, 2, 0, col, half);
    sin[1] = load_nat<f16x8>(a.hash_nat, wt, 2, 1, col, half);
    float v[2][8];
    f16x8 tc[2];
    bf16x8 tc_b[2];
    time_values<2, false>(a.t, half, v);
    cast_values<2>(v, tc, tc_b);
    sin[2] = tc[0]; sin[3] = tc[1];
  }
  template <bool TRAIN>
  static __device__ __forceinline__ void operands(const CanonArgs& a, int64_t wt, int64_t nc, int col, int half, f16x8 (&sin)[4], f16x8 (&denc)[2]) {
    bf16x8 sin_b[4], denc_b[2];
    sin[0] = load_nat<f16x8>(a.hash_nat, wt, 2, 0, col, half);
    sin[1] = load_nat<f16x8>(a.hash_nat, wt, 2, 1, col, half);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) sin_b[ks][j] = (__bf16)(float)sin[ks][j];
    {
      float v[2][8];
      f16x8 tc[2];
      bf16x8 tc_b[2];
      time_values<2, false>(a.t[nc], half, v);                      // bias-free network: the pad columns stay zero
      cast_values<2>(v, tc, tc_b);
      sin[2] = tc[0]; sin[3] = tc[1];
      sin_b[2] = tc_b[0]; sin_b[3] = tc_b[1];
      dir_values<2>(a.dirs[nc * 3 + 0], a.dirs[nc * 3 + 1], a.dirs[nc * 3 + 2], half, v);
      cast_values<2>(v, denc, denc_b);
    }
    if constexpr (TRAIN) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) stash_nat(a.sin_nat, wt, 4, ks, col, half, sin_b[ks]);
      stash_nat(a.denc, wt, 2, 0, col, half, denc_b[0]);
      stash_nat(a.denc, wt, 2, 1, col, half, denc_b[1]);
    }
  }
};

template <bool TRAIN>
__global__ void __launch_bounds__(kThreads) canon_fwd_kernel(const CanonArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  instant_forward<CanonPolicy, TRAIN>(a, smem, tid, lane, wave, col, half);
}

// The canonical chain of the Part 3 evaluation launch chain (nerf_p3_render_rays_fwd): instant_forward<., false> on the first *count
// rows at ONE time stamp, count and time both read from DEVICE memory.  The policy is CanonPolicy with the time code formed from the
// scalar, by sigma_operands' calls; inference stores no image, so the struct carries the image names as NULLs only.
struct CanonScalarArgs {
  const char* packed;
  const __bf16* hash_nat;  // nat [roundup(capacity, 128),32] FP16 at x_c (hash_fwd_counted_f16)
  float t;                 // set by the kernel from its time word
  const float* dirs;       // [capacity,3] unit view directions
  int64_t n, n_pad;        // set by the kernel from its count word
  float* rgb; float* sigma;
  __bf16* hs1; __bf16* hc1; __bf16* hc2;   // never dereferenced (TRAIN = false)
};
struct CanonScalarPolicy : CanonPolicy {
  template <bool TRAIN>
  static __device__ __forceinline__ void operands(const CanonScalarArgs& a, int64_t wt, int64_t nc, int col, int half, f16x8 (&sin)[4], f16x8 (&denc)[2]) {
    static_assert(!TRAIN, "the scalar-time canonical chain is inference only");
    sin[0] = load_nat<f16x8>(a.hash_nat, wt, 2, 0, col, half);
    sin[1] = load_nat<f16x8>(a.hash_nat, wt, 2, 1, col, half);
    float v[2][8];
    f16x8 tc[2];
    bf16x8 tc_b[2], denc_b[2];
    time_values<2, false>(a.t, half, v);
    cast_values<2>(v, tc, tc_b);
    sin[2] = tc[0]; sin[3] = tc[1];
    dir_values<2>(a.dirs[nc * 3 + 0], a.dirs[nc * 3 + 1], a.dirs[nc * 3 + 2], half, v);
    cast_values<2>(v, denc, denc_b);
  }
};

// The launch is sized for `capacity` rows; the count is clamped to it (a count the compaction cannot produce must not become an access
// outside the chunk's pieces), n == 0 leaves before n - 1 exists, n_pad is formed here.
__global__ void __launch_bounds__(kThreads) canon_fwd_counted_kernel(const CanonScalarArgs a0, const unsigned* __restrict__ count,
                                                                     int64_t capacity, const float* __restrict__ time_dev) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int64_t n = (int64_t)*count;
  if (n == 0) return;
  n = n < capacity ? n : capacity;
  CanonScalarArgs a = a0;
  a.t = *time_dev;
  a.n = n;
  a.n_pad = (n + kTile - 1) / kTile * kTile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  instant_forward<CanonScalarPolicy, false>(a, smem, tid, lane, wave, col, half);
}

__global__ void __launch_bounds__(kThreads) canon_bwd_kernel(const CanonArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  instant_dgrad<CanonPolicy>(a, smem, tid, lane, wave, col, half);
}

// The canonical chain of the occupancy-grid refresh (nerf_p4_grid_update): the sigma-net alone (S1, S2: 12 of the forward's 30
// fragments) on a slab's hash image at x_c and the time code of one anchor, folded into the grid as a running maximum
struct CanonSigmaArgs {
  const char* packed;
  const __bf16* hash_nat;   // nat [n_pad,32] FP16 of the slab's x_c
  float t;                  // the anchor
  int64_t n, n_pad;
  float* grid;              // [n] in/out, the slab's cells
  uint8_t* binary;          // [n]
  float decay; int dynamic; float threshold;
  unsigned long long* count;   // NULL: this pass does not count
};
constexpr int kCanonSigmaFrags = step_of(C1).frag0 - kCanonFwd0;

__global__ void __launch_bounds__(kThreads) canon_sigma_grid_kernel(const CanonSigmaArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  instant_sigma<CanonPolicy>(a, smem, tid, lane, wave, col, half);
}

// ------------------------------------------------------------------------------------------------ per-sample inputs
// t' and x' of every compacted sample (core.py:289-297): t = times[ray of the sample]; training with use_coord_noise
// adds N(0, std) noise from the counter-based generator, keyed by (seed, counter) and the sample's index in the
// GLOBAL batch (first_sample + g), so data-parallel shards draw what one GPU would
__device__ __forceinline__ void normal_pair(uint64_t counter, uint64_t index, uint64_t key, float& z0, float& z1) {
  const float u1 = fmaxf(squares_uniform(counter, 2 * index, key), 5.9604644775390625e-08f);
  const float u2 = squares_uniform(counter, 2 * index + 1, key);
  const float r = sqrtf(-2.0f * __logf(u1));
  z0 = r * __builtin_amdgcn_sinf(u2 + 0.25f);      // v_sin_f32 takes revolutions: cos(2 pi u2)
  z1 = r * __builtin_amdgcn_sinf(u2);
}

__global__ void __launch_bounds__(256)
prep_kernel(const int* __restrict__ slots, const float* __restrict__ pts, const float* __restrict__ times, int64_t total, int S,
            float std_x, float std_t, uint64_t key, uint64_t counter, uint64_t first_sample,
            float* __restrict__ x_out, float* __restrict__ t_out) {
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    const int slot = slots != nullptr ? slots[g] : (int)g;
    if (slot < 0) continue;
    float t = times[S > 0 ? g / S : g];
    float x[3] = {pts[(int64_t)slot * 3 + 0], pts[(int64_t)slot * 3 + 1], pts[(int64_t)slot * 3 + 2]};
    if (std_x > 0.0f || std_t > 0.0f) {
      float z0, z1, z2, z3;
      normal_pair(counter, 2 * (first_sample + (uint64_t)g), key, z0, z1);
      normal_pair(counter, 2 * (first_sample + (uint64_t)g) + 1, key, z2, z3);
      if (std_x > 0.0f) { x[0] += z0 * std_x; x[1] += z1 * std_x; x[2] += z2 * std_x; }
      if (std_t > 0.0f) t = fminf(fmaxf(t + z3 * std_t, 0.0f), 1.0f);
    }
    if (x_out != nullptr) { x_out[(int64_t)slot * 3 + 0] = x[0]; x_out[(int64_t)slot * 3 + 1] = x[1]; x_out[(int64_t)slot * 3 + 2] = x[2]; }
    t_out[slot] = t;
  }
}

struct Layout {
  int64_t n_pad;
  size_t feat[3], canon_nat, tc, ht1, tm, df, hd1, hd2, dmask, wts, raw, dzt1, dzt2, dzd1, dzd2, dsmall_d, dfeat[3];
  size_t sin_nat, hs1, h16, denc, hc1, hc2, cmask, dzs1, dzs2, dzc1, dzc2, dsmall_c, dfeat_c, sum_ws, slab, total;
};
static Layout layout(int64_t n) {
  Layout s{};
  s.n_pad = (n + kTile - 1) / kTile * kTile;
  const size_t np = (size_t)s.n_pad;
  size_t o = 0;
  for (int k = 0; k < 3; ++k) s.feat[k] = take(&o, np * 32 * 2);
  s.canon_nat = take(&o, np * 32 * 2);
  s.tc = take(&o, np * 32 * 2); s.ht1 = take(&o, np * 64 * 2); s.tm = take(&o, np * 64 * 2); s.df = take(&o, np * 32 * 2);
  s.hd1 = take(&o, np * 64 * 2); s.hd2 = take(&o, np * 64 * 2); s.dmask = take(&o, (np / kTile) * kThreads * 16);
  s.wts = take(&o, np * 16); s.raw = take(&o, np * 12);
  s.dzt1 = take(&o, np * 64 * 2); s.dzt2 = take(&o, np * 64 * 2); s.dzd1 = take(&o, np * 64 * 2); s.dzd2 = take(&o, np * 64 * 2);
  s.dsmall_d = take(&o, np * 16 * 2);
  for (int k = 0; k < 3; ++k) s.dfeat[k] = take(&o, np * kHashDeform * 4);
  s.sin_nat = take(&o, np * 64 * 2); s.hs1 = take(&o, np * 64 * 2); s.h16 = take(&o, np * 32 * 2); s.denc = take(&o, np * 32 * 2);
  s.hc1 = take(&o, np * 64 * 2); s.hc2 = take(&o, np * 64 * 2); s.cmask = take(&o, (np / kTile) * kThreads * 16);
  s.dzs1 = take(&o, np * 64 * 2); s.dzs2 = take(&o, np * 32 * 2); s.dzc1 = take(&o, np * 64 * 2); s.dzc2 = take(&o, np * 64 * 2);
  s.dsmall_c = take(&o, np * 16 * 2); s.dfeat_c = take(&o, np * 32 * 4);
  // option "deterministic": ordered sum of the displacement-scale gradient, partial tiles of the weight-gradient launches
  s.sum_ws = take(&o, ordered_sum_ws_words(1) * sizeof(unsigned)); s.slab = take(&o, kSmallSlabBytes);
  s.total = o;
  return s;
}

static DeformArgs deform_args(const void* packed, const float* params, void* ws, int64_t n) {
  const Layout l = layout(n);
  char* w = static_cast<char*>(ws);
  auto B = [&](size_t off) { return reinterpret_cast<__bf16*>(w + off); };
  DeformArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.params = params; a.n = n; a.n_pad = l.n_pad;
  for (int k = 0; k < 3; ++k) { a.feat[k] = B(l.feat[k]); a.d_feat[k] = reinterpret_cast<float*>(w + l.dfeat[k]); }
  a.tc = B(l.tc); a.ht1 = B(l.ht1); a.tm = B(l.tm); a.df = B(l.df); a.hd1 = B(l.hd1); a.hd2 = B(l.hd2);
  a.mask = reinterpret_cast<uint4*>(w + l.dmask);
  a.wts = reinterpret_cast<float*>(w + l.wts); a.raw = reinterpret_cast<float*>(w + l.raw);
  a.dzt1 = B(l.dzt1); a.dzt2 = B(l.dzt2); a.dzd1 = B(l.dzd1); a.dzd2 = B(l.dzd2); a.dsmall = B(l.dsmall_d);
  return a;
}

static CanonArgs canon_args(const void* packed, void* ws, int64_t n) {
  const Layout l = layout(n);
  char* w = static_cast<char*>(ws);
  auto B = [&](size_t off) { return reinterpret_cast<__bf16*>(w + off); };
  CanonArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.n = n; a.n_pad = l.n_pad;
  a.hash_nat = B(l.canon_nat); a.sin_nat = B(l.sin_nat); a.hs1 = B(l.hs1); a.h16 = B(l.h16); a.denc = B(l.denc);
  a.hc1 = B(l.hc1); a.hc2 = B(l.hc2); a.mask = reinterpret_cast<uint4*>(w + l.cmask);
  a.dzs1 = B(l.dzs1); a.dzs2 = B(l.dzs2); a.dzc1 = B(l.dzc1); a.dzc2 = B(l.dzc2); a.dsmall = B(l.dsmall_c);
  a.d_feat = reinterpret_cast<float*>(w + l.dfeat_c);
  return a;
}

}  // namespace p4
}  // namespace nerf

using namespace nerf;
using namespace nerf::p4;

extern "C" int64_t nerf_p4_param_count(void) { return kParams; }
extern "C" size_t nerf_p4_packed_bytes(void) { return kPackBytes; }
extern "C" size_t nerf_p4_workspace_bytes(int64_t n) { return n > 0 ? layout(n).total : 0; }
// what train == 0 touches: the four operand images lead the layout (slots 0..3); nothing behind them is read or written
extern "C" size_t nerf_p4_infer_workspace_bytes(int64_t n) { return n > 0 ? layout(n).tc : 0; }
extern "C" size_t nerf_p4_workspace_offset(int64_t n, int which) {
  if (n <= 0) return 0;
  const Layout l = layout(n);
  switch (which) {
    case 0: case 1: case 2: return l.feat[which];        // nat images of the three deformation grids (hash forward outputs)
    case 3: return l.canon_nat;                            // nat image of the canonical grid at x_c
    case 4: case 5: case 6: return l.dfeat[which - 4];    // d features of the three deformation grids [n,24] fp32
    case 7: return l.dfeat_c;                              // d features of the canonical grid [n,32] fp32
    default: return (size_t)-1;
  }
}

extern "C" int nerf_p4_pack(const float* params_f32, void* packed, nerf_stream_t stream) {
  NERF_REQUIRE(params_f32 && packed && ((uintptr_t)packed & 255) == 0, "nerf_p4_pack: bad pointer");
  hipLaunchKernelGGL(p4::pack_kernel, dim3(32), dim3(256), 0, as_stream(stream), params_f32, static_cast<char*>(packed));
  return check_launch("nerf_p4_pack");
}

extern "C" int nerf_p4_sample_inputs(const int* slot_of_sample, const float* pts_compact, const float* ray_times, int64_t n_rays,
                                     int n_samples, float coord_noise_std, float time_noise_std, uint64_t seed, uint64_t counter,
                                     int64_t first_ray, float* x_deform, float* t_deform, nerf_stream_t stream) {
  NERF_REQUIRE(n_rays >= 0 && n_samples >= 0 && first_ray >= 0 && counter < ((uint64_t)1 << 24), "nerf_p4_sample_inputs: bad sizes");
  // four draws per sample (indices 4 g .. 4 g + 3 of the counter's stream), each below 2^40 where the next counter's stream begins
  constexpr int64_t kSampleLimit = (int64_t)1 << 38;
  NERF_REQUIRE(first_ray < kSampleLimit && n_rays < kSampleLimit &&
                   first_ray + n_rays <= (kSampleLimit - 1) / (int64_t)(n_samples > 0 ? n_samples : 1),
               "nerf_p4_sample_inputs: (first_ray + n_rays) * max(n_samples, 1) must stay below 2^38");
  const int64_t total = n_samples > 0 ? n_rays * n_samples : n_rays;
  if (total == 0) return NERF_OK;
  NERF_REQUIRE(pts_compact && ray_times && t_deform, "nerf_p4_sample_inputs: NULL pointer");
  NERF_REQUIRE(n_samples == 0 || slot_of_sample != nullptr, "nerf_p4_sample_inputs: slot map is NULL");
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(p4::prep_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), slot_of_sample, pts_compact, ray_times, total,
                     n_samples, coord_noise_std, time_noise_std, squares_key(seed ^ 0x6e6f697365ull), counter,   // its own stream: the depth jitter of
                                                                                                     // nerf_sample_compact_jitter draws from squares_key(seed)
                     (uint64_t)first_ray * (uint64_t)(n_samples > 0 ? n_samples : 1), x_deform, t_deform);
  return check_launch("nerf_p4_sample_inputs");
}

extern "C" int nerf_p4_deform_fwd(const void* packed, const float* params_f32, void* workspace, const float* pts, const float* t_deform,
                                  const float* blend, int64_t n, float* delta_x, float* x_canonical, int train, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0, "nerf_p4_deform_fwd: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && params_f32 && workspace && pts && t_deform && delta_x && x_canonical && ((uintptr_t)workspace & 255) == 0,
               "nerf_p4_deform_fwd: bad pointer");
  DeformArgs a = deform_args(packed, params_f32, workspace, n);
  a.t = t_deform; a.blend = blend; a.x = pts; a.dx = delta_x; a.xc = x_canonical;
  const int grid = grid_for(a.n_pad / kTile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p4_deform_fwd: cannot query device");
  const int lds = kDeformFwdN * 1024 + 256;
  if (train) hipLaunchKernelGGL(p4::deform_fwd_kernel<true>, dim3(grid), dim3(kThreads), lds, as_stream(stream), a);
  else hipLaunchKernelGGL(p4::deform_fwd_kernel<false>, dim3(grid), dim3(kThreads), lds, as_stream(stream), a);
  return check_launch("nerf_p4_deform_fwd");
}

extern "C" int nerf_p4_canon_fwd(const void* packed, void* workspace, const float* t_deform, const float* dirs, int64_t n, float* rgb,
                                 float* sigma, int train, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0, "nerf_p4_canon_fwd: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && workspace && t_deform && dirs && rgb && sigma && ((uintptr_t)workspace & 255) == 0, "nerf_p4_canon_fwd: bad pointer");
  CanonArgs a = canon_args(packed, workspace, n);
  a.t = t_deform; a.dirs = dirs; a.rgb = rgb; a.sigma = sigma;
  const int grid = grid_for(a.n_pad / kTile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p4_canon_fwd: cannot query device");
  if (train) hipLaunchKernelGGL(p4::canon_fwd_kernel<true>, dim3(grid), dim3(kThreads), kCanonFwdN * 1024, as_stream(stream), a);
  else hipLaunchKernelGGL(p4::canon_fwd_kernel<false>, dim3(grid), dim3(kThreads), kCanonFwdN * 1024, as_stream(stream), a);
  return check_launch("nerf_p4_canon_fwd");
}

// Backward of the canonical chain: d_feat (workspace slot 7) = d loss / d hash features; the five weight gradients are
// ACCUMULATED into grads_f32 (the caller zeroes the vector once per step: several passes -- data batch, regulariser
// probes -- add into it)
extern "C" int nerf_p4_canon_bwd(const void* packed, void* workspace, const float* rgb, const float* sigma, const float* d_rgb,
                                 const float* d_sigma, int64_t n, float* grads_f32, void* amax_bits, void* grad_lm, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && grads_f32, "nerf_p4_canon_bwd: bad arguments");
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && workspace && rgb && sigma && d_rgb && d_sigma, "nerf_p4_canon_bwd: NULL pointer");
  CanonArgs a = canon_args(packed, workspace, n);
  a.rgb = const_cast<float*>(rgb); a.sigma = const_cast<float*>(sigma); a.d_rgb = d_rgb; a.d_sigma = d_sigma;
  a.amax_bits = static_cast<unsigned*>(amax_bits); a.grad_lm = static_cast<float2*>(grad_lm);
  const int grid = grid_for(a.n_pad / kTile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p4_canon_bwd: cannot query device");
  hipLaunchKernelGGL(p4::canon_bwd_kernel, dim3(grid), dim3(kThreads), kCanonBwdN * 1024, as_stream(stream), a);
  if (int rc = check_launch("nerf_p4_canon_bwd (dgrad)"); rc != NERF_OK) return rc;
  const Layout l = layout(n);
  const char* w = static_cast<const char*>(workspace);
  WgradArgs wa{};
  { WgradJob j = make_job(w, l.dzs1, 4096, 2, 0, 0, l.sin_nat, 2, 12); j.w_off = kS1; j.w_ld = 64; j.o_valid = 64; j.nat_valid = 32 + kTimeDim; wa.jobs[0] = j; }
  instant_common_jobs(wa, w, InstantImages{l.hs1, l.h16, l.denc, l.hc1, l.hc2, l.dzs2, l.dzc1, l.dzc2, l.dsmall_c}, kS2, kC1, kC2, kC3);
  wa.n_jobs = 5;
  if (options().deterministic)
    return wgrad_launch(wa, n, grads_f32, as_stream(stream), reinterpret_cast<float*>(const_cast<char*>(w) + l.slab), kSmallSlabBytes);
  return wgrad_launch(wa, n, grads_f32, as_stream(stream));
}

// Backward of the deformation chain from d loss / d delta_x: d features of the three grids (workspace slots 4..6, already
// multiplied by the blend weights), the time-modulation and displacement-decoder weight gradients and the gradient of
// displacement_scale ACCUMULATED into grads_f32
extern "C" int nerf_p4_deform_bwd(const void* packed, const float* params_f32, void* workspace, const float* d_delta_x, int64_t n,
                                  float* grads_f32, void* amax_bits, void* grad_lm, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && grads_f32, "nerf_p4_deform_bwd: bad arguments");
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && params_f32 && workspace && d_delta_x, "nerf_p4_deform_bwd: NULL pointer");
  DeformArgs a = deform_args(packed, params_f32, workspace, n);
  a.d_dx = d_delta_x; a.g_scale = grads_f32 + kScale; a.amax_bits = static_cast<unsigned*>(amax_bits);
  a.grad_lm = static_cast<float2*>(grad_lm);
  const int grid = grid_for(a.n_pad / kTile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p4_deform_bwd: cannot query device");
  const bool det = options().deterministic != 0;
  const Layout l = layout(n);
  if (det) {
    NERF_REQUIRE(grid <= kOrderedSumMaxBlocks, "nerf_p4_deform_bwd: %d workgroups (ordered sum: at most %d)", grid, kOrderedSumMaxBlocks);
    a.sum_ws = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + l.sum_ws);
    if (hipMemsetAsync(a.sum_ws, 0, sizeof(unsigned) * kOrderedSumTickets, as_stream(stream)) != hipSuccess)
      return fail(NERF_ELAUNCH, "nerf_p4_deform_bwd: memset failed");
  }
  hipLaunchKernelGGL(p4::deform_bwd_kernel, dim3(grid), dim3(kThreads), kDeformBwdN * 1024, as_stream(stream), a);
  if (int rc = check_launch("nerf_p4_deform_bwd (dgrad)"); rc != NERF_OK) return rc;
  const char* w = static_cast<const char*>(workspace);
  WgradArgs wa{};
  { WgradJob j = make_job(w, l.dzt1, 4096, 2, 0, 0, l.tc, 1, 6); j.w_off = kT1W; j.w_ld = 21; j.o_valid = 64; j.nat_valid = kTimeDim;
    j.bias_off = kT1b; j.bias_nat_col = kTimeDim; wa.jobs[0] = j; }
  { WgradJob j = make_job(w, l.dzt2, 4096, 2, l.ht1, 2, 0, 0, 10); j.ones = 1; j.w_off = kT2W; j.w_ld = 64; j.o_valid = 64; j.acc_valid = 64;
    j.bias_off = kT2b; wa.jobs[1] = j; }
  { WgradJob j = make_job(w, l.dzd1, 4096, 2, l.tm, 2, l.df, 1, 11); j.w_off = kD1; j.w_ld = 96; j.o_valid = 64; j.acc_valid = 64;
    j.acc_col0 = kHashDeform; j.nat_valid = kHashDeform; j.nat_col0 = 0; wa.jobs[2] = j; }
  { WgradJob j = make_job(w, l.dzd2, 4096, 2, l.hd1, 2, 0, 0, 7); j.w_off = kD2; j.w_ld = 64; j.o_valid = 64; j.acc_valid = 64; wa.jobs[3] = j; }
  { WgradJob j = make_job(w, l.dsmall_d, 1024, 1, l.hd2, 2, 0, 0, 9); j.a_nat = 1; j.split_n = 1; j.w_off = kD3; j.w_ld = 64; j.o_valid = 3; j.acc_valid = 64; wa.jobs[4] = j; }
  wa.n_jobs = 5;
  if (det) return wgrad_launch(wa, n, grads_f32, as_stream(stream), reinterpret_cast<float*>(static_cast<char*>(workspace) + l.slab), kSmallSlabBytes);
  return wgrad_launch(wa, n, grads_f32, as_stream(stream));
}

// The chain launches of nerf_p4_grid_update per (slab, anchor) (common.h; grid.hip has checked the entry's arguments)
int nerf::p4_deform_lattice(const void* packed, const float* params_f32, const void* feat_nat, float t, int64_t cell0, int64_t n_cells,
                            int resolution, float grid_bound, float* x_canonical, nerf_stream_t stream) {
  NERF_REQUIRE(cell0 >= 0 && n_cells > 0 && resolution >= 2 && packed && params_f32 && feat_nat && x_canonical, "p4_deform_lattice: bad arguments");
  DeformLatticeArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.feat = static_cast<const __bf16*>(feat_nat);
  a.params = params_f32; a.t = t;
  a.cell0 = cell0; a.n = n_cells; a.n_pad = (n_cells + kTile - 1) / kTile * kTile;
  a.res = resolution; a.bound = grid_bound; a.step = lattice_step(grid_bound, resolution);
  a.xc = x_canonical;
  const int grid = grid_for(a.n_pad / kTile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p4_grid_update: cannot query device");
  hipLaunchKernelGGL(p4::deform_lattice_kernel, dim3(grid), dim3(kThreads), kDeformLatticeN * 1024, as_stream(stream), a);
  return check_launch("nerf_p4_grid_update (deformation chain)");
}

int nerf::p4_canon_sigma_grid(const void* packed, const void* hash_nat, float t, int64_t n_cells, float* grid, uint8_t* binary_grid, float decay,
                              float threshold, unsigned long long* active_count, nerf_stream_t stream) {
  NERF_REQUIRE(n_cells > 0 && packed && hash_nat && grid && binary_grid, "p4_canon_sigma_grid: bad arguments");
  CanonSigmaArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.hash_nat = static_cast<const __bf16*>(hash_nat);
  a.t = t; a.n = n_cells; a.n_pad = (n_cells + kTile - 1) / kTile * kTile;
  a.grid = grid; a.binary = binary_grid; a.decay = decay; a.dynamic = 1; a.threshold = threshold; a.count = active_count;
  // two workgroups per CU, one atomic per workgroup: imlp_sigma_grid's launch shape (DESIGN 4.22 measured both)
  const int wgs = grid_for(a.n_pad / kTile, 2);
  if (wgs <= 0) return fail(NERF_ELAUNCH, "nerf_p4_grid_update: cannot query device");
  hipLaunchKernelGGL(p4::canon_sigma_grid_kernel, dim3(wgs), dim3(kThreads), kCanonSigmaFrags * 1024, as_stream(stream), a);
  return check_launch("nerf_p4_grid_update (sigma-net)");
}

// The canonical launch of nerf_p3_render_rays_fwd per chunk (common.h; render_p3.hip has checked the entry's arguments):
// nerf_p4_canon_fwd's launch shape sized for the chunk's capacity, surplus workgroups fall out of the striding tile loop.
int nerf::p4_canon_fwd_counted(const void* packed, const void* hash_nat, const float* dirs, const unsigned* count, int64_t capacity,
                               const float* time_dev, float* rgb, float* sigma, nerf_stream_t stream) {
  NERF_REQUIRE(capacity > 0 && packed && hash_nat && dirs && count && time_dev && rgb && sigma, "p4_canon_fwd_counted: bad arguments");
  CanonScalarArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.hash_nat = static_cast<const __bf16*>(hash_nat);
  a.dirs = dirs; a.rgb = rgb; a.sigma = sigma;
  const int grid = grid_for((capacity + kTile - 1) / kTile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p3_render_rays_fwd: cannot query device");
  hipLaunchKernelGGL(p4::canon_fwd_counted_kernel, dim3(grid), dim3(kThreads), kCanonFwdN * 1024, as_stream(stream), a, count, capacity, time_dev);
  return check_launch("nerf_p3_render_rays_fwd (canonical chain)");
}
