// What the resident-weight tiny-MLP chains (imlp.hip, p4mlp.hip, p3deform.hip, imlp_shapes.hip) share: the step record, the
// fragment pack loop, the LDS prologue, the step runner, the ReLU-bit and masked-gradient epilogues, the small operands and the
// Instant-NGP head.
//
// The chain: 32 samples per wave on the MFMA column, accumulator tiles -> 16-bit B fragments of the next step, EVERY weight
// fragment of one direction copied to LDS once per launch and read from there by every tile (neither the two-slot ring of
// mlp_chain.h nor the per-step staging of sample_chain.h).  Each engine keeps its step table, its pack source map, its kernels,
// its job table and its C entries; every __global__ entry point stays in its own file and namespace.
#pragma once
#include "mlp_chain.h"

namespace nerf {
namespace resident {

// (m-tiles, k-steps fed by the previous step's accumulators, natural-order k-steps, first fragment of the packed image)
struct Step { int mt, ks_acc, ks_nat, frag0; };
typedef Step (*StepFn)(int);

// ------------------------------------------------------------------------------------------------ packing
// Fragments 0..n_frags-1 of a packed image, by the whole grid: fragment -> (step, m-tile, k-step), lane -> (row, eight columns in
// the step's k order), src_of(step, row, k, nat) -> the flat parameter index or -1 (structural zero), rounded to fp16 where
// is_fp16(step) and to bf16 elsewhere.  step_of(s) must have ascending frag0.  first / stride: the grid-stride
// loop's bounds, formed in the __global__ caller (blockDim read in a device function keeps the select for a partial last workgroup).
template <class StepOf, class SrcOf, class IsFp16>
__device__ __forceinline__ void pack_fragments(const float* __restrict__ params, char* __restrict__ packed, int n_frags, int n_steps,
                                               StepOf step_of, SrcOf src_of, IsFp16 is_fp16, int first, int stride) {
  for (int t = first; t < n_frags * 64; t += stride) {
    const int frag = t >> 6, lane = t & 63;
    int step = 0;
    for (int s = 0; s < n_steps; ++s) if (frag >= step_of(s).frag0) step = s;
    const Step st = step_of(step);
    const int ksn = st.ks_acc + st.ks_nat, rel = frag - st.frag0, mt = rel / ksn, ks = rel % ksn;
    const int row = mt * 32 + (lane & 31), h = lane >> 5;
    const bool nat = ks >= st.ks_acc, f16 = is_fp16(step);
    unsigned short out[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int src = src_of(step, row, frag_column(nat ? ks - st.ks_acc : ks, h, j, nat), nat);
      const float v = src >= 0 ? params[src] : 0.0f;
      out[j] = f16 ? __builtin_bit_cast(unsigned short, (_Float16)v) : __builtin_bit_cast(unsigned short, (__bf16)v);
    }
    store_fragment(packed, frag, lane, out);
  }
}

// ------------------------------------------------------------------------------------------------ prologue and step runner
// fragments [frag0, frag0 + n_frags) of the packed image -> LDS from smem on, by a workgroup of THREADS; returns this lane's A
// base, rebased so that the step tables' frag0 (which count from the start of the image) index it.  The caller's barrier follows.
// tid / lane: the __global__ wrapper's (read from threadIdx again here, the tile loops came out with other registers).
template <int THREADS>
__device__ __forceinline__ const char* resident_weights(char* smem, const char* packed, int frag0, int n_frags, int tid, int lane) {
  for (int i = tid; i < n_frags * 64; i += THREADS)
    reinterpret_cast<uint4*>(smem)[i] = reinterpret_cast<const uint4*>(packed + frag0 * 1024)[i];
  return smem + lane * 16 - frag0 * 1024;
}

// every m-tile of step STEP of table STEP_OF: acc = bias (or 0) + A B, then epi(integral_constant m, acc).  V / mfma: bf16x8 with
// MfmaBf, f16x8 with Mfma16.  FENCE: one tile at a time (interleaved tiles cost registers at 4 m-tiles of 8 k-steps).
template <StepFn STEP_OF, int STEP, int KS, bool FENCE = false, class V, class F, class Epi>
__device__ __forceinline__ void run_step(const char* wbase, const V (&b)[KS], const float* bias_lds, F mfma, Epi&& epi) {
  constexpr Step st = STEP_OF(STEP);
  static_assert(KS == st.ks_acc + st.ks_nat, "k-steps");
  const int half = (threadIdx.x & 63) >> 5;
  static_for<st.mt>([&](auto mc) {
    constexpr int m = decltype(mc)::value;
    f32x16 acc;
    if (bias_lds != nullptr) acc = bias_tile(bias_lds, 32 * m, half);
    else {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    }
    acc = mtile<KS>(wbase, st.frag0 + m * KS, b, acc, mfma);
    epi(mc, acc);
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
  });
}

// ------------------------------------------------------------------------------------------------ operands and epilogues
__device__ __forceinline__ void to_operand(const f32x16& acc, bf16x8& lo, bf16x8& hi) { acc_to_operand(acc, lo, hi); }
__device__ __forceinline__ void to_operand(const f32x16& acc, f16x8& lo, f16x8& hi) { acc_to_operand16(acc, lo, hi); }

// natural-order k-step ks of a [wave tile][n_ks][1 KiB] image (what stash_nat wrote, or the hash forward), as bf16 or fp16 bits
template <class V>
__device__ __forceinline__ V load_nat(const __bf16* img, int64_t wt, int n_ks, int ks, int col, int half) {
  return *reinterpret_cast<const V*>(reinterpret_cast<const char*>(img) + ((wt * n_ks + ks) * 64 + 2 * col + half) * 16);
}
// the two B fragments of m-tile m of a blocked image (what stash_block wrote)
__device__ __forceinline__ void load_block(const __bf16* img, int64_t wt, int n_mtiles, int m, int col, int half, bf16x8& lo, bf16x8& hi) {
  const char* p = reinterpret_cast<const char*>(img) + (wt * n_mtiles + m) * 2048 + block_lane_offset(col, half);
  lo = *reinterpret_cast<const bf16x8*>(p);
  hi = *reinterpret_cast<const bf16x8*>(p + 128);
}
// blocked bf16 training image of an accumulator tile whose operand fragments are lo / hi (bf16: those; fp16: rounded again from acc)
template <class V>
__device__ __forceinline__ void stash_tile(__bf16* stash, int64_t wt, int n_mtiles, int m, int col, int half, const f32x16& acc,
                                           const V& lo, const V& hi) {
  if constexpr (std::is_same<V, bf16x8>::value) stash_block(stash, wt, n_mtiles, m, col, half, lo, hi);
  else {
    bf16x8 l, h;
    acc_to_operand(acc, l, h);
    stash_block(stash, wt, n_mtiles, m, col, half, l, h);
  }
}

// the 16-wide natural operand that carries three output derivatives on lane-half 0 (columns 0..2), zero elsewhere
__device__ __forceinline__ bf16x8 small_operand(float g0, float g1, float g2, int half) {
  bf16x8 small;
#pragma unroll
  for (int j = 0; j < 8; ++j) small[j] = (__bf16)0.0f;
  if (half == 0) { small[0] = (__bf16)g0; small[1] = (__bf16)g1; small[2] = (__bf16)g2; }
  return small;
}

// ReLU in place; bit r of the result: accumulator register r was positive
__device__ __forceinline__ uint32_t relu_mask(f32x16& acc) {
  uint32_t bits = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) { bits |= (acc[r] > 0.0f ? 1u : 0u) << r; acc[r] = fmaxf(acc[r], 0.0f); }
  return bits;
}
__device__ __forceinline__ void mask_grad(f32x16& acc, uint32_t bits) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = (bits >> r) & 1u ? acc[r] : 0.0f;
}
// epilogue of a ReLU layer of up to two m-tiles: operand fragments out[2m], out[2m+1] of the next step, the tile's 16 mask bits
// into half-word m of `word`, and (TRAIN) the blocked bf16 image
template <bool TRAIN, class V>
__device__ __forceinline__ auto relu_epilogue(V* out, __bf16* stash, uint32_t& word, int64_t wt, int col, int half) {
  return [=, &word](auto mc, f32x16 acc) {
    constexpr int m = decltype(mc)::value;
    word |= relu_mask(acc) << (16 * m);
    to_operand(acc, out[2 * m], out[2 * m + 1]);
    if constexpr (TRAIN) stash_tile(stash, wt, 2, m, col, half, acc, out[2 * m], out[2 * m + 1]);
  };
}
// epilogue of a transposed ReLU layer: the gradient where the forward's bit is set, as the next operand and as a blocked image
__device__ __forceinline__ auto grad_epilogue(bf16x8* out, __bf16* stash, uint32_t bits32, int64_t wt, int col, int half) {
  return [=](auto mc, f32x16 acc) {
    constexpr int m = decltype(mc)::value;
    mask_grad(acc, bits32 >> (16 * m));
    acc_to_operand(acc, out[2 * m], out[2 * m + 1]);
    stash_block(stash, wt, 2, m, col, half, out[2 * m], out[2 * m + 1]);
  };
}

// ------------------------------------------------------------------------------------------------ Instant-NGP head
// sigma = softplus(h[0] - 5) (reference src/decoders.py:153; F.softplus with its threshold of 20)
__device__ __forceinline__ float head_sigma(float h0) {
  const float x = h0 - 5.0f;
  return x > 20.0f ? x : log1pf(expf(x));
}
__device__ __forceinline__ void head_rgb_store(float* rgb, int64_t n, const f32x16& acc) {
#pragma unroll
  for (int c = 0; c < 3; ++c) rgb[n * 3 + c] = 1.0f / (1.0f + __expf(-acc[c]));
}
// derivatives of the loss at the pre-activations: g[0..2] through the sigmoid, g[3] through the softplus
// (softplus'(x) = sigmoid(x) = 1 - exp(-softplus(x)): no cancellation); zero for a pad sample
template <class A>
__device__ __forceinline__ void head_derivs(const A& a, int64_t n, bool live, float (&g)[4]) {
  g[0] = g[1] = g[2] = g[3] = 0.0f;
  if (live) {
    const float r0 = a.rgb[n * 3 + 0], r1 = a.rgb[n * 3 + 1], r2 = a.rgb[n * 3 + 2];
    g[0] = a.d_rgb[n * 3 + 0] * r0 * (1.0f - r0);
    g[1] = a.d_rgb[n * 3 + 1] * r1 * (1.0f - r1);
    g[2] = a.d_rgb[n * 3 + 2] * r2 * (1.0f - r2);
    g[3] = a.d_sigma[n] * -expm1f(-a.sigma[n]);
  }
}

}  // namespace resident
}  // namespace nerf
