// Instant-NGP decoder at the shapes the YAML allows (reference src/decoders.py:100-162 behind NeuralField('part2_instant')): the
// two bias-free tiny MLPs of imlp.hip with the widths as parameters,
//   sigma-net  2L -> H (relu) -> 16 (linear);  sigma = softplus(h[0] - 5)
//   colour-net [h (16) | dir code (D)] -> H (relu) -> H (relu) -> 3 (sigmoid)          D = 3 + 6 L_embed_dir
// Compiled: n_levels L = 1..16 at 2 features per level, hidden_dim H = 32 / 64 / 128 (1, 2 or 4 m-tiles of the 32x32x16 bf16
// MFMA), L_embed_dir 0..4.  The kernels are templated on H; L and L_embed_dir are run-time values of the plan: the hash operand
// and the direction code always take two natural-order k-steps, whose columns past 2L (past D) are structural zeros of the
// weight fragments.
//
// The register chain is imlp.hip's, step for step and k-step for k-step, on the shared pieces of resident_chain.h (32 samples per
// wave on the MFMA column, accumulator tiles -> bf16 B fragments, every weight fragment resident in LDS for the whole launch:
// 68 KiB forward at H = 128; pack loop, LDS prologue, fenced step runner, the Instant head), with the same rounding points --
// bf16 hash features, direction code, post-ReLU activations, h16 and gradient images, fp32 accumulation, sigma and rgb -- and the
// same softplus, softplus' (-expm1f(-sigma)) and sigmoid formulas: at (16, 64, 4) the forward and the feature gradients carry
// imlp.hip's bits.
//
// The hash forward writes columns 0..2L-1 of its operand image only (hashgrid.hip: n_ks = ceil(2L / 16) k-steps per wave tile):
// columns 2L..16 n_ks - 1 may hold anything, NaN included, and a zero weight does not remove a NaN.  They are cleared by a select
// on load.  Every other image column this file reads was written by this file.
//
// Training images are row-major bf16 (sample_chain.h): hash features [n_pad][32], [h16 | dir code] [n_pad][48], hs1 / hc1 / hc2
// [n_pad][H]; the ReLU masks are one bit per activation.  The dgrad kernel runs the transposed chain, writes the pre-activation
// gradient images and d_feat [n, 2L] fp32 row-major (what the counted hash backward reads).  Weight gradients: chunk-partial
// tiles over the sample axis (sample_chain.h::wgrad_job with this decoder's job table), then one reduction in chunk order, which
// also writes the exact zeros of the pad rows and columns.  No float atomics anywhere: the same bits on every run.
//
// tools/kernel_resources.py ishape:: lists the registers (scratch 0 and no spills in every kernel).
//
// Parameter vector (fp32, [out, in] row-major, bias-free) = decoders.tiny_mlp_shapes:
//   sigma_net : W1 [H, pad16(2L)] | W2 [16, H]
//   color_net : W1 [H, pad16(16 + D)] | W2 [H, H] | W3 [16, H] (rows 3..15 unused)
#include <math.h>
#include "resident_chain.h"
#include "sample_chain.h"

namespace nerf {
namespace ishape {
using namespace sample_chain;
using namespace resident;

constexpr int kThreads = 256, kTile = 128;
constexpr int kHashLd = 32, kCatLd = 48, kH16Ld = 16, kSmallLd = 8;
constexpr int kMaxLevels = 16, kMaxLd = 4;

struct Plan {
  int H, L, Ld, F, P1, D, P2;                       // F = 2L hash features, P1 = pad16(F); D direction columns, P2 = pad16(16 + D)
  int sw1, sw2, cw1, cw2, cw3, n_params, slab_stride;
};

// NULL, or the key this build is not compiled for
static const char* make_plan(int L, int H, int Ld, Plan* p) {
  if (L < 1 || L > kMaxLevels) return "n_levels";
  if (!(H == 32 || H == 64 || H == 128)) return "hidden_dim";
  if (Ld < 0 || Ld > kMaxLd) return "L_embed_dir";
  *p = Plan{};
  p->H = H; p->L = L; p->Ld = Ld; p->F = 2 * L; p->P1 = (p->F + 15) / 16 * 16; p->D = 3 + 6 * Ld; p->P2 = (16 + p->D + 15) / 16 * 16;
  p->sw1 = 0; p->sw2 = H * p->P1; p->cw1 = p->sw2 + 16 * H; p->cw2 = p->cw1 + H * p->P2; p->cw3 = p->cw2 + H * H;
  p->n_params = p->cw3 + 16 * H; p->slab_stride = (p->n_params + 63) / 64 * 64;
  return nullptr;
}

// fragment plan of one H; forward steps 0..4 = S1 S2 C1 C2 C3, backward 5..9 = C3t C2t C1t S2t S1t (imlp.hip::istep at H = 64)
__host__ __device__ constexpr Step step_of(int H, int s) {
  const int MT = H / 32, KS = H / 16;
  const int mt[10] = {MT, 1, MT, MT, 1, MT, MT, 1, MT, 1};
  const int ka[10] = {0, KS, 1, KS, KS, 0, KS, KS, 1, KS};
  const int kn[10] = {2, 0, 2, 0, 0, 1, 0, 0, 0, 0};
  int f = 0;
  for (int i = 0; i < s; ++i) f += mt[i] * (ka[i] + kn[i]);
  return {mt[s], ka[s], kn[s], f};
}
template <int H>
constexpr Step step_h(int s) { return step_of(H, s); }
__host__ __device__ constexpr int fwd_frags(int H) { return step_of(H, 5).frag0; }
__host__ __device__ constexpr int all_frags(int H) { return step_of(H, 9).frag0 + H / 16; }
static size_t packed_bytes(const Plan& p) { return (size_t)all_frags(p.H) * 1024; }

// flat parameter index feeding A[row][k] of a step, or -1 for a structural zero; nat: k counts the natural-order columns
__device__ __forceinline__ int src_index(const Plan& p, int step, int row, int k, bool nat) {
  const int H = p.H;
  switch (step) {
    case 0: return k < p.F ? p.sw1 + row * p.P1 + k : -1;
    case 1: return row < 16 ? p.sw2 + row * H + k : -1;
    case 2: return nat ? (k < p.D ? p.cw1 + row * p.P2 + 16 + k : -1) : (k < 16 ? p.cw1 + row * p.P2 + k : -1);
    case 3: return p.cw2 + row * H + k;
    case 4: return row < 3 ? p.cw3 + row * H + k : -1;
    case 5: return k < 3 ? p.cw3 + k * H + row : -1;
    case 6: return p.cw2 + k * H + row;
    case 7: return row < 16 ? p.cw1 + k * p.P2 + row : -1;
    case 8: return k < 16 ? p.sw2 + k * H + row : -1;
    default: return row < p.F ? p.sw1 + k * p.P1 + row : -1;
  }
}

__global__ void __launch_bounds__(256) pack_kernel(const float* __restrict__ params, char* __restrict__ packed, const Plan p) {
  pack_fragments(params, packed, all_frags(p.H), 10, [&](int s) { return step_of(p.H, s); },
                 [&](int step, int row, int k, bool nat) { return src_index(p, step, row, k, nat); }, [](int) { return false; },
                 blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

struct Args {
  const char* packed;
  Plan p;
  const __bf16* hash_nat;    // nat blocks [n_pad / 32][n_ks][1 KiB] from nerf_hash_encode_fwd, n_ks = ceil(2L / 16)
  const float* dirs;         // [n,3] unit view directions
  int64_t n, n_pad;
  float* rgb;                // [n,3]
  float* sigma;              // [n]
  __bf16* xin; __bf16* cat; __bf16* hs1; __bf16* hc1; __bf16* hc2;        // training images (row-major)
  unsigned* mask;            // [tiles][256][3 mask_words(H)]
  const float* d_rgb; const float* d_sigma;                               // backward
  __bf16* dzs1; __bf16* dzs2; __bf16* dzc1; __bf16* dzc2; __bf16* dsmall;
  float* d_feat;             // [n, 2L] fp32
};

constexpr int mask_words(int H) { return (H / 32 + 1) / 2; }             // 16 ReLU bits per m-tile and lane
// bit r: the tile's bf16 activation of accumulator register r is non-zero (r < 8: lo[r], else hi[r - 8]).  The values are
// post-ReLU, sign bit clear: h + 0x7fff carries into bit 15 exactly when the half-word h is non-zero, and never past it.
// (Sixteen compares of the fp32 accumulators against zero cost the training forward 80 more registers: spills at H = 128.)
__device__ __forceinline__ uint32_t relu_bits16(const bf16x8& lo, const bf16x8& hi) {
  const u32x4 wl = __builtin_bit_cast(u32x4, lo), wh = __builtin_bit_cast(u32x4, hi);
  uint32_t bits = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t tl = wl[q] + 0x7fff7fffu, th = wh[q] + 0x7fff7fffu;
    bits |= (((tl >> 15) & 1u) | ((tl >> 30) & 2u)) << (2 * q);
    bits |= (((th >> 15) & 1u) | ((th >> 30) & 2u)) << (8 + 2 * q);
  }
  return bits;
}

// the two natural-order k-steps of the hash features of wave tile wt: feature f = 16 ks + 8 half + j, CLEARED from 2L on (the
// hash forward does not write those columns of its image, and has no second k-step at all when 2L <= 16)
__device__ __forceinline__ void hash_operand(const __bf16* img, int64_t wt, int F, int col, int half, bf16x8 (&out)[2]) {
  const int n_ks = (F + 15) >> 4;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    u32x4 w = {0u, 0u, 0u, 0u};
    if (ks < n_ks) w = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(img) + ((wt * n_ks + ks) * 64 + 2 * col + half) * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = 16 * ks + 8 * half + 2 * q < F ? w[q] : 0u;     // F is even: a word is two valid features or none
    out[ks] = __builtin_bit_cast(bf16x8, w);
  }
}

// the two natural-order k-steps of the direction code (fourier.hip's arithmetic, formed in registers: mlp_chain.h)
__device__ __forceinline__ void dir_operand(const float* d, int Ld, int half, bf16x8 (&out)[2]) {
  const float x = d[0], y = d[1], z = d[2];
  switch (Ld) {
    case 0: fourier_operand<2, 3>(x, y, z, half, out); break;
    case 1: fourier_operand<2, 9>(x, y, z, half, out); break;
    case 2: fourier_operand<2, 15>(x, y, z, half, out); break;
    case 3: fourier_operand<2, 21>(x, y, z, half, out); break;
    default: fourier_operand<2, 27>(x, y, z, half, out); break;
  }
}

// rows 0..15 of an accumulator tile as one bf16 fragment `lo` (features 8 g + 4 half + (0..3), g = 0, 1) -> 16 row-major columns
__device__ __forceinline__ void store_rows16(__bf16* img, int ld, int64_t n, int half, const bf16x8& lo) {
  __bf16* row = img + n * ld + 4 * half;
  *reinterpret_cast<bf16x4*>(row + 0) = bf16x4{lo[0], lo[1], lo[2], lo[3]};
  *reinterpret_cast<bf16x4*>(row + 8) = bf16x4{lo[4], lo[5], lo[6], lo[7]};
}

template <int H, bool TRAIN>
__global__ void __launch_bounds__(kThreads, 2) fwd_kernel(const Args a) {
  constexpr int KS = H / 16, MW = mask_words(H), FR = fwd_frags(H);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = resident_weights<kThreads>(smem, a.packed, 0, FR, tid, lane);
  __syncthreads();
  const int64_t n_tiles = a.n_pad / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t wt = tile * 4 + wave, n = wt * 32 + col;
    const bool live = n < a.n;
    const int64_t nc = live ? n : a.n - 1;
    bf16x8 hin[2], denc[2];
    hash_operand(a.hash_nat, wt, a.p.F, col, half, hin);
    dir_operand(a.dirs + nc * 3, a.p.Ld, half, denc);
    if constexpr (TRAIN) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        *reinterpret_cast<bf16x8*>(a.xin + n * kHashLd + 16 * ks + 8 * half) = hin[ks];
        *reinterpret_cast<bf16x8*>(a.cat + n * kCatLd + 16 + 16 * ks + 8 * half) = denc[ks];
      }
    }
    uint32_t mw[3 * MW];
#pragma unroll
    for (int i = 0; i < 3 * MW; ++i) mw[i] = 0u;
    auto relu_epi = [&](bf16x8* out, __bf16* img, int layer) {
      return [=, &mw](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.0f);
        acc_to_operand(acc, out[2 * m], out[2 * m + 1]);
        if constexpr (TRAIN) mw[layer * MW + (m >> 1)] |= relu_bits16(out[2 * m], out[2 * m + 1]) << (16 * (m & 1));
        if constexpr (TRAIN) store_rows(img, H, n, m, half, out[2 * m], out[2 * m + 1]);
      };
    };
    bf16x8 hs1[KS], h16[2], hc1[KS], hc2[KS];
    run_step<step_h<H>, 0, 2, true>(wbase, hin, nullptr, MfmaBf{}, relu_epi(hs1, a.hs1, 0));
    float h0 = 0.0f;
    run_step<step_h<H>, 1, KS, true>(wbase, hs1, nullptr, MfmaBf{}, [&](auto, f32x16 acc) {
      h0 = acc[0];
      acc_to_operand(acc, h16[0], h16[1]);            // rows 16..31 of this tile are structural zeros: h16[1] is not used
      if constexpr (TRAIN) store_rows16(a.cat, kCatLd, n, half, h16[0]);
    });
    if (live && half == 0) a.sigma[n] = head_sigma(h0);
    {
      bf16x8 cat[3] = {h16[0], denc[0], denc[1]};
      run_step<step_h<H>, 2, 3, true>(wbase, cat, nullptr, MfmaBf{}, relu_epi(hc1, a.hc1, 1));
    }
    run_step<step_h<H>, 3, KS, true>(wbase, hc1, nullptr, MfmaBf{}, relu_epi(hc2, a.hc2, 2));
    run_step<step_h<H>, 4, KS, true>(wbase, hc2, nullptr, MfmaBf{}, [&](auto, f32x16 acc) {
      if (live && half == 0) head_rgb_store(a.rgb, n, acc);
    });
    if constexpr (TRAIN) {
      unsigned* mp = a.mask + (tile * kThreads + tid) * (3 * MW);
#pragma unroll
      for (int i = 0; i < 3 * MW; ++i) mp[i] = mw[i];
    }
  }
}

template <int H>
__global__ void __launch_bounds__(kThreads, 2) dgrad_kernel(const Args a) {
  constexpr int KS = H / 16, MW = mask_words(H), FR = fwd_frags(H), BR = all_frags(H) - FR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = resident_weights<kThreads>(smem, a.packed, FR, BR, tid, lane);     // step_of().frag0 counts from the forward stream
  __syncthreads();
  const int64_t n_tiles = a.n_pad / kTile;
  const int F = a.p.F;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t wt = tile * 4 + wave, n = wt * 32 + col;
    const bool live = n < a.n;
    float g[4];
    head_derivs(a, n, live, g);
    bf16x8 small;
#pragma unroll
    for (int j = 0; j < 8; ++j) small[j] = (__bf16)0.0f;
    if (half == 0) {                                           // small_operand, and its row-major image from the same lanes
      small[0] = (__bf16)g[0]; small[1] = (__bf16)g[1]; small[2] = (__bf16)g[2];
      *reinterpret_cast<bf16x8*>(a.dsmall + n * kSmallLd) = small;
    }
    uint32_t mw[3 * MW];
    {
      const unsigned* mp = a.mask + (tile * kThreads + tid) * (3 * MW);
#pragma unroll
      for (int i = 0; i < 3 * MW; ++i) mw[i] = mp[i];
    }
    auto grad_epi = [&](bf16x8* out, __bf16* img, int layer) {
      return [=, &mw](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
        mask_grad(acc, mw[layer * MW + (m >> 1)] >> (16 * (m & 1)));
        acc_to_operand(acc, out[2 * m], out[2 * m + 1]);
        store_rows(img, H, n, m, half, out[2 * m], out[2 * m + 1]);
      };
    };
    bf16x8 gc2[KS], gc1[KS], g16[2], gs1[KS];
    { bf16x8 in[1] = {small}; run_step<step_h<H>, 5, 1, true>(wbase, in, nullptr, MfmaBf{}, grad_epi(gc2, a.dzc2, 2)); }
    run_step<step_h<H>, 6, KS, true>(wbase, gc2, nullptr, MfmaBf{}, grad_epi(gc1, a.dzc1, 1));
    run_step<step_h<H>, 7, KS, true>(wbase, gc1, nullptr, MfmaBf{}, [&](auto, f32x16 acc) {
      if (half == 0) acc[0] += g[3];                             // row 0 of h also feeds sigma
      acc_to_operand(acc, g16[0], g16[1]);
      store_rows16(a.dzs2, kH16Ld, n, half, g16[0]);
    });
    { bf16x8 in[1] = {g16[0]}; run_step<step_h<H>, 8, 1, true>(wbase, in, nullptr, MfmaBf{}, grad_epi(gs1, a.dzs1, 0)); }
    run_step<step_h<H>, 9, KS, true>(wbase, gs1, nullptr, MfmaBf{}, [&](auto, f32x16 acc) {
      if (!live) return;
      // registers 4g..4g+3 = features 8g + 4 half + (0..3); a row of d_feat is 8L bytes: 8-byte stores, columns below 2L only
      float* row = a.d_feat + n * F;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int f = 8 * g + 4 * half;
        if (f < F) *reinterpret_cast<float2*>(row + f) = make_float2(acc[4 * g], acc[4 * g + 1]);
        if (f + 2 < F) *reinterpret_cast<float2*>(row + f + 2) = make_float2(acc[4 * g + 2], acc[4 * g + 3]);
      }
    });
  }
}

// Weight gradients (sample_chain.h::wgrad_job); a chunk's slab row has the layout of the parameter vector.  blockIdx.x: chunk,
// blockIdx.y: job.
struct WgradArgs {
  Plan p;
  const __bf16* xin; const __bf16* cat; const __bf16* hs1; const __bf16* hc1; const __bf16* hc2;
  const __bf16* dzs1; const __bf16* dzs2; const __bf16* dzc1; const __bf16* dzc2; const __bf16* dsmall;
  int64_t n, chunk;
  float* slab;               // [chunks][slab_stride]
};
// jobs: S1 x blocks | C1 x blocks | C2 x blocks | S2 | C3, blocks of kOBlock output features
__host__ __device__ inline int job_count(const Plan& p) { return 3 * ((p.H + kOBlock - 1) / kOBlock) + 2; }
__device__ __forceinline__ Job job_of(const WgradArgs& a, int job) {
  const Plan& p = a.p;
  const int H = p.H, blocks = (H + kOBlock - 1) / kOBlock;
  Job j{};
  j.b_off = -1;
  if (job < 3 * blocks) {
    const int which = job / blocks;
    j.a_ld = H; j.O = H; j.o0 = (job % blocks) * kOBlock;
    if (which == 0) { j.A = a.dzs1; j.B = a.xin; j.b_ld = kHashLd; j.I = p.F; j.w_off = p.sw1; j.w_ld = p.P1; }
    else if (which == 1) { j.A = a.dzc1; j.B = a.cat; j.b_ld = kCatLd; j.I = 16 + p.D; j.w_off = p.cw1; j.w_ld = p.P2; }
    else { j.A = a.dzc2; j.B = a.hc1; j.b_ld = H; j.I = H; j.w_off = p.cw2; j.w_ld = H; }
    return j;
  }
  j.o0 = 0; j.b_ld = H; j.I = H; j.w_ld = H;
  if (job == 3 * blocks) { j.A = a.dzs2; j.a_ld = kH16Ld; j.O = 16; j.B = a.hs1; j.w_off = p.sw2; }
  else { j.A = a.dsmall; j.a_ld = kSmallLd; j.O = 3; j.B = a.hc2; j.w_off = p.cw3; }
  return j;
}
__global__ void __launch_bounds__(256) wgrad_kernel(const WgradArgs a) {
  const Job jb = job_of(a, blockIdx.y);
  const int64_t n0 = blockIdx.x * a.chunk;
  const int64_t n1 = n0 + a.chunk < a.n ? n0 + a.chunk : a.n;
  wgrad_job(jb, n0, n1, a.slab + (size_t)blockIdx.x * a.p.slab_stride);
}

// is flat parameter q a real weight (the jobs store these), or a pad row / column of tiny_mlp_shapes (never stored)?
__device__ __forceinline__ bool is_weight(const Plan& p, int q) {
  if (q < p.sw2) return q % p.P1 < p.F;
  if (q < p.cw1) return true;
  if (q < p.cw2) return (q - p.cw1) % p.P2 < 16 + p.D;
  if (q < p.cw3) return true;
  return (q - p.cw3) / p.H < 3;
}
// grads[q] = sum over chunks, in chunk order; pad rows and columns: exactly zero
__global__ void __launch_bounds__(256) reduce_kernel(const float* __restrict__ slab, int chunks, const Plan p, float* __restrict__ grads) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < p.n_params) grads[q] = is_weight(p, q) ? ordered_sum(slab, chunks, p.slab_stride, q) : 0.0f;
}

struct Layout {
  int64_t n_pad;
  size_t hash_nat, xin, cat, hs1, hc1, hc2, mask, dzs1, dzs2, dzc1, dzc2, dsmall, slab, total;
};
static Layout layout(const Plan& p, int64_t n) {
  Layout s{};
  s.n_pad = (n + kTile - 1) / kTile * kTile;
  const size_t np = (size_t)s.n_pad, H = (size_t)p.H;
  size_t o = 0;
  int64_t chunk, chunks;
  chunking(n, &chunk, &chunks);
  s.hash_nat = take(&o, np * kHashLd * 2);          // the hash forward fills ceil(2L / 16) of its two k-steps
  s.xin = take(&o, np * kHashLd * 2);
  s.cat = take(&o, np * kCatLd * 2);
  s.hs1 = take(&o, np * H * 2);
  s.hc1 = take(&o, np * H * 2);
  s.hc2 = take(&o, np * H * 2);
  s.mask = take(&o, (np / kTile) * kThreads * 3 * mask_words(p.H) * 4);
  s.dzs1 = take(&o, np * H * 2);
  s.dzs2 = take(&o, np * kH16Ld * 2);
  s.dzc1 = take(&o, np * H * 2);
  s.dzc2 = take(&o, np * H * 2);
  s.dsmall = take(&o, np * kSmallLd * 2);
  s.slab = take(&o, (size_t)chunks * p.slab_stride * 4);
  s.total = o;
  return s;
}

static Args args_of(const Plan& p, const void* packed, void* ws, int64_t n) {
  const Layout l = layout(p, n);
  char* w = static_cast<char*>(ws);
  auto img = [&](size_t off) { return reinterpret_cast<__bf16*>(w + off); };
  Args a{};
  a.packed = static_cast<const char*>(packed); a.p = p; a.n = n; a.n_pad = l.n_pad;
  a.hash_nat = img(l.hash_nat);
  a.xin = img(l.xin); a.cat = img(l.cat); a.hs1 = img(l.hs1); a.hc1 = img(l.hc1); a.hc2 = img(l.hc2);
  a.mask = reinterpret_cast<unsigned*>(w + l.mask);
  a.dzs1 = img(l.dzs1); a.dzs2 = img(l.dzs2); a.dzc1 = img(l.dzc1); a.dzc2 = img(l.dzc2); a.dsmall = img(l.dsmall);
  return a;
}

typedef void (*ChainKernel)(Args);
static ChainKernel fwd_kernel_of(int H, bool train) {
  switch (H) {
    case 32: return train ? fwd_kernel<32, true> : fwd_kernel<32, false>;
    case 64: return train ? fwd_kernel<64, true> : fwd_kernel<64, false>;
    default: return train ? fwd_kernel<128, true> : fwd_kernel<128, false>;
  }
}
static ChainKernel dgrad_kernel_of(int H) { return H == 32 ? dgrad_kernel<32> : (H == 64 ? dgrad_kernel<64> : dgrad_kernel<128>); }
static int launch(ChainKernel kernel, const Args& a, int frags, nerf_stream_t stream, const char* what) {
  const int grid = grid_for(a.n_pad / kTile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "%s: cannot query device", what);
  return launch_chain(kernel, grid, kThreads, frags * 1024, stream, what, a);
}

}  // namespace ishape
}  // namespace nerf

using namespace nerf;

#define ISHAPE int n_levels, int hidden_dim, int L_embed_dir
#define ISHAPE_PLAN(what)                                                                                                              \
  ishape::Plan plan;                                                                                                                   \
  if (const char* key = ishape::make_plan(n_levels, hidden_dim, L_embed_dir, &plan))                                                   \
    return fail(NERF_EINVAL, what ": %s is not compiled (n_levels=%d hidden_dim=%d L_embed_dir=%d; compiled: n_levels 1..16 at 2 "     \
                "features per level, hidden_dim 32/64/128, L_embed_dir 0..4)", key, n_levels, hidden_dim, L_embed_dir)

extern "C" int64_t nerf_imlp_shape_param_count(ISHAPE) {
  ishape::Plan plan;
  if (const char* key = ishape::make_plan(n_levels, hidden_dim, L_embed_dir, &plan)) {
    fail(NERF_EINVAL, "nerf_imlp_shape_param_count: %s is not compiled (n_levels=%d hidden_dim=%d L_embed_dir=%d)", key, n_levels,
         hidden_dim, L_embed_dir);
    return -1;
  }
  return plan.n_params;
}
extern "C" size_t nerf_imlp_shape_packed_bytes(ISHAPE) {
  ishape::Plan plan;
  return ishape::make_plan(n_levels, hidden_dim, L_embed_dir, &plan) == nullptr ? ishape::packed_bytes(plan) : 0;
}
extern "C" size_t nerf_imlp_shape_workspace_bytes(int64_t n, ISHAPE) {
  ishape::Plan plan;
  return n > 0 && ishape::make_plan(n_levels, hidden_dim, L_embed_dir, &plan) == nullptr ? ishape::layout(plan, n).total : 0;
}
extern "C" size_t nerf_imlp_shape_hash_operand_offset(int64_t n, ISHAPE) {
  ishape::Plan plan;
  return n > 0 && ishape::make_plan(n_levels, hidden_dim, L_embed_dir, &plan) == nullptr ? ishape::layout(plan, n).hash_nat : 0;
}

extern "C" int nerf_imlp_shape_pack(const float* params_f32, ISHAPE, void* packed, nerf_stream_t stream) {
  ISHAPE_PLAN("nerf_imlp_shape_pack");
  NERF_REQUIRE(params_f32 && packed && ((uintptr_t)packed & 255) == 0, "nerf_imlp_shape_pack: bad pointer");
  hipLaunchKernelGGL(ishape::pack_kernel, dim3((ishape::all_frags(plan.H) * 64 + 255) / 256), dim3(256), 0, as_stream(stream), params_f32,
                     static_cast<char*>(packed), plan);
  return check_launch("nerf_imlp_shape_pack");
}

extern "C" int nerf_imlp_shape_fwd(const void* packed, void* workspace, const float* dirs, int64_t n, ISHAPE, float* rgb, float* sigma,
                                   int train, nerf_stream_t stream) {
  ISHAPE_PLAN("nerf_imlp_shape_fwd");
  NERF_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "nerf_imlp_shape_fwd: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && workspace && dirs && rgb && sigma && ((uintptr_t)workspace & 255) == 0 && ((uintptr_t)packed & 255) == 0,
               "nerf_imlp_shape_fwd: bad pointer");
  ishape::Args a = ishape::args_of(plan, packed, workspace, n);
  a.dirs = dirs; a.rgb = rgb; a.sigma = sigma;
  return ishape::launch(ishape::fwd_kernel_of(plan.H, train != 0), a, ishape::fwd_frags(plan.H), stream, "nerf_imlp_shape_fwd");
}

extern "C" int nerf_imlp_shape_bwd(const void* packed, void* workspace, const float* rgb, const float* sigma, const float* d_rgb,
                                   const float* d_sigma, int64_t n, ISHAPE, float* grads_f32, float* d_feat, nerf_stream_t stream) {
  ISHAPE_PLAN("nerf_imlp_shape_bwd");
  NERF_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && grads_f32, "nerf_imlp_shape_bwd: bad arguments");
  if (n == 0) {
    if (hipMemsetAsync(grads_f32, 0, sizeof(float) * plan.n_params, as_stream(stream)) != hipSuccess)
      return fail(NERF_ELAUNCH, "nerf_imlp_shape_bwd: memset failed");
    return NERF_OK;
  }
  NERF_REQUIRE(packed && workspace && rgb && sigma && d_rgb && d_sigma && d_feat && ((uintptr_t)workspace & 255) == 0 &&
               ((uintptr_t)packed & 255) == 0 && ((uintptr_t)d_feat & 7) == 0, "nerf_imlp_shape_bwd: bad pointer");
  const ishape::Layout l = ishape::layout(plan, n);
  ishape::Args a = ishape::args_of(plan, packed, workspace, n);
  a.rgb = const_cast<float*>(rgb); a.sigma = const_cast<float*>(sigma); a.d_rgb = d_rgb; a.d_sigma = d_sigma; a.d_feat = d_feat;
  int rc = ishape::launch(ishape::dgrad_kernel_of(plan.H), a, ishape::all_frags(plan.H) - ishape::fwd_frags(plan.H), stream,
                          "nerf_imlp_shape_bwd (dgrad)");
  if (rc != NERF_OK) return rc;
  int64_t chunk, chunks;
  ishape::chunking(n, &chunk, &chunks);
  ishape::WgradArgs g{};
  g.p = plan; g.xin = a.xin; g.cat = a.cat; g.hs1 = a.hs1; g.hc1 = a.hc1; g.hc2 = a.hc2;
  g.dzs1 = a.dzs1; g.dzs2 = a.dzs2; g.dzc1 = a.dzc1; g.dzc2 = a.dzc2; g.dsmall = a.dsmall;
  g.n = n; g.chunk = chunk; g.slab = reinterpret_cast<float*>(static_cast<char*>(workspace) + l.slab);
  hipLaunchKernelGGL(ishape::wgrad_kernel, dim3((unsigned)chunks, (unsigned)ishape::job_count(plan)), dim3(256), 0, as_stream(stream), g);
  if (rc = check_launch("nerf_imlp_shape_bwd (wgrad)"); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(ishape::reduce_kernel, dim3((plan.n_params + 255) / 256), dim3(256), 0, as_stream(stream), g.slab, (int)chunks,
                     plan, grads_f32);
  return check_launch("nerf_imlp_shape_bwd (reduce)");
}
