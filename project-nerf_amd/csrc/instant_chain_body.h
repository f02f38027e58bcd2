// The kernel bodies (forward, density only, dgrad) of the Instant-NGP decoder at its default shape (sigma-net 64 -> 16, colour-net [16 | 32] -> 64 -> 64 -> 3),
// on the blocks of resident_chain.h.  imlp.hip (Part 2, bf16 operands, hash features only) and p4mlp.hip's canonical chain (Part 4,
// fp16 forward operands, [hash | time code] into the sigma-net) instantiate them; each keeps its __global__ wrappers, argument
// struct, step table and C entries.  imlp_shapes.hip (row-major images, wider masks, run-time widths) keeps its own bodies.
//
// A policy P supplies what differs:
//   P::step_of, P::S1 .. P::S1t      the file's step table and the ten step indices
//   P::kFwd0/kFwdN, P::kBwd0/kBwdN   fragment ranges of the two directions in the packed image
//   P::V, P::Mfma                    forward operand vector and MFMA (bf16x8 / MfmaBf, f16x8 / Mfma16)
//   P::kSigmaKs                      natural k-steps of the sigma-net's input
//   P::operands<TRAIN>(a, wt, nc, col, half, sin, denc)   forms both inputs and (TRAIN) writes their bf16 images
//   P::sigma_operands(a, wt, col, half, sin)              forms the sigma-net's input alone (instant_sigma; only where it is instantiated)
//   P::kFence                        forward: run_step's FENCE (one m-tile at a time)
//   P::kZeroGrads (P::kParams)       the dgrad kernel clears a.zero_grads[0, kParams) for the weight-gradient launch behind it
// The argument struct is passed BY VALUE and tid .. half are formed in the __global__ wrapper (by reference, the
// fields were reloaded inside the tile loop; formed here, the indices cost scalar registers).
#pragma once
#include "resident_chain.h"

namespace nerf {
namespace resident {

constexpr int kInstantThreads = 256, kInstantTile = 128;

template <class P, bool TRAIN, class A>
__device__ __forceinline__ void instant_forward(const A a, char* smem, int tid, int lane, int wave, int col, int half) {
  using V = typename P::V;
  const typename P::Mfma mfma{};
  const char* wbase = resident_weights<kInstantThreads>(smem, a.packed, P::kFwd0, P::kFwdN, tid, lane);
  __syncthreads();
  const int64_t n_tiles = a.n_pad / kInstantTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t wt = tile * 4 + wave, n = wt * 32 + col;
    const bool live = n < a.n;
    const int64_t nc = live ? n : a.n - 1;
    V sin[P::kSigmaKs], denc[2];
    P::template operands<TRAIN>(a, wt, nc, col, half, sin, denc);
    uint32_t mw[3] = {0, 0, 0};
    V hs1[4], h16[2], hc1[4], hc2[4];
    run_step<P::step_of, P::S1, P::kSigmaKs, P::kFence>(wbase, sin, nullptr, mfma, relu_epilogue<TRAIN>(hs1, a.hs1, mw[0], wt, col, half));
    float h0 = 0.0f;
    run_step<P::step_of, P::S2, 4, P::kFence>(wbase, hs1, nullptr, mfma, [&](auto, f32x16 acc) {
      h0 = acc[0];
      to_operand(acc, h16[0], h16[1]);
      if constexpr (TRAIN) stash_tile(a.h16, wt, 1, 0, col, half, acc, h16[0], h16[1]);
    });
    if (live && half == 0) a.sigma[n] = head_sigma(h0);
    {
      V cat[3] = {h16[0], denc[0], denc[1]};
      run_step<P::step_of, P::C1, 3, P::kFence>(wbase, cat, nullptr, mfma, relu_epilogue<TRAIN>(hc1, a.hc1, mw[1], wt, col, half));
    }
    run_step<P::step_of, P::C2, 4, P::kFence>(wbase, hc1, nullptr, mfma, relu_epilogue<TRAIN>(hc2, a.hc2, mw[2], wt, col, half));
    run_step<P::step_of, P::C3, 4, P::kFence>(wbase, hc2, nullptr, mfma, [&](auto, f32x16 acc) {
      if (live && half == 0) head_rgb_store(a.rgb, n, acc);
    });
    if constexpr (TRAIN) a.mask[tile * kInstantThreads + tid] = make_uint4(mw[0], mw[1], mw[2], 0);
  }
}

// Density only, folded into an occupancy grid (nerf_instant_grid_update): instant_forward's geometry, S1 and S2 alone -- the same
// operands, MFMAs and fence, so h0 is the forward's bit for bit; no direction code, no colour-net, no stash, no mask.  Only the
// fragments of S1 and S2 are resident: the prefix of the forward fragment stream (P::step_of(S2) ends it).  Row n of the image is
// cell n of a.grid / a.binary (the caller offsets both to the slab's first cell).  Epilogue = grid_update_kernel's arithmetic
// (grid.hip; reference src/renderer.py:118-132) on the lane that owns acc[0] of a live row; every thread counts its active cells
// over its whole tile loop: one reduction and one 64-bit atomic per workgroup at the kernel's end, none per tile.
// P adds: P::sigma_operands(a, wt, col, half, sin) forms the sigma-net's input alone.
// A: packed, n, n_pad, grid, binary, decay, dynamic, threshold, count (NULL: nothing is counted) (+ what P::sigma_operands reads).
template <class P, class A>
__device__ __forceinline__ void instant_sigma(const A a, char* smem, int tid, int lane, int wave, int col, int half) {
  using V = typename P::V;
  const typename P::Mfma mfma{};
  constexpr Step s2 = P::step_of(P::S2);
  constexpr int kFrags = s2.frag0 + s2.mt * (s2.ks_acc + s2.ks_nat) - P::kFwd0;
  static_assert(P::step_of(P::S1).frag0 == P::kFwd0 && kFrags > 0 && kFrags <= P::kFwdN, "S1, S2 lead the forward fragment stream");
  const char* wbase = resident_weights<kInstantThreads>(smem, a.packed, P::kFwd0, kFrags, tid, lane);
  __syncthreads();
  const int64_t n_tiles = a.n_pad / kInstantTile;
  unsigned long long active = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t wt = tile * 4 + wave, n = wt * 32 + col;
    const bool live = n < a.n;
    V sin[P::kSigmaKs];
    P::sigma_operands(a, wt, col, half, sin);
    uint32_t mw = 0;
    V hs1[4];
    run_step<P::step_of, P::S1, P::kSigmaKs, P::kFence>(wbase, sin, nullptr, mfma, relu_epilogue<false>(hs1, (__bf16*)nullptr, mw, wt, col, half));
    float h0 = 0.0f;
    run_step<P::step_of, P::S2, 4, P::kFence>(wbase, hs1, nullptr, mfma, [&](auto, f32x16 acc) { h0 = acc[0]; });
    if (live && half == 0) {
      float v = head_sigma(h0);
      if (a.dynamic) v = fmaxf(a.grid[n] * a.decay, v);
      a.grid[n] = v;
      const bool on = v > a.threshold;
      a.binary[n] = on ? 1 : 0;
      active += on ? 1 : 0;
    }
  }
  // one wave reduction, then ONE 64-bit atomic per workgroup: with one per wave (grid_update_kernel's form) the 4096 same-address
  // atomics of a 2^18-cell slab, retiring one after the other in L2, were the kernel -- 53.8 us against 17.6 us for the whole decoder
  // on the same rows
  for (int off = 32; off > 0; off >>= 1) active += __shfl_xor(active, off);
  __shared__ unsigned long long wave_active[kInstantThreads / 64];
  if (lane == 0) wave_active[wave] = active;
  __syncthreads();
  if (tid == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kInstantThreads / 64; ++w) total += wave_active[w];
    if (total && a.count != nullptr) atomicAdd(a.count, total);      // NULL: a pass whose cells a later pass counts (nerf_p4_grid_update)
  }
}

// d loss / d hash features of one sample from the last transposed step's tile: row-major [n,32] fp32, or (a.grad_lm) level-major
// [16][n] float2, and the running largest magnitude for the hash scatter's fixed-point scale
template <class A>
__device__ __forceinline__ void feat_grad_store(const A& a, int64_t n, int half, const f32x16& acc, float& amax) {
  if (a.grad_lm != nullptr) {
    // registers 4g..4g+3 = features 8g + 4 half + (0..3) = levels 4g + 2 half and + 1: two float2 per group, each store
    // instruction covers 32 consecutive points of one level (256 contiguous bytes)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int lvl = 4 * g + 2 * half;
      a.grad_lm[(int64_t)lvl * a.n + n] = make_float2(acc[4 * g], acc[4 * g + 1]);
      a.grad_lm[(int64_t)(lvl + 1) * a.n + n] = make_float2(acc[4 * g + 2], acc[4 * g + 3]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) amax = fmaxf(amax, fabsf(acc[r]));
    return;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
    *reinterpret_cast<f32x4*>(a.d_feat + n * 32 + 8 * g + 4 * half) = v;
  }
  if (a.amax_bits != nullptr) {
#pragma unroll
    for (int r = 0; r < 16; ++r) amax = fmaxf(amax, fabsf(acc[r]));
  }
}

template <class P, class A>
__device__ __forceinline__ void instant_dgrad(const A a, char* smem, int tid, int lane, int wave, int col, int half) {
  const MfmaBf mfma{};
  const char* wbase = resident_weights<kInstantThreads>(smem, a.packed, P::kBwd0, P::kBwdN, tid, lane);
  __syncthreads();
  const int64_t n_tiles = a.n_pad / kInstantTile;
  if constexpr (P::kZeroGrads) {                                // instead of a fill launch before this one (4.5 us + its gap)
    if (a.zero_grads != nullptr)
      for (int i = blockIdx.x * kInstantThreads + tid; i < P::kParams; i += gridDim.x * kInstantThreads) a.zero_grads[i] = 0.0f;
  }
  float amax = 0.0f;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t wt = tile * 4 + wave, n = wt * 32 + col;
    const bool live = n < a.n;
    float g[4];
    head_derivs(a, n, live, g);
    const bf16x8 small = small_operand(g[0], g[1], g[2], half);
    stash_nat(a.dsmall, wt, 1, 0, col, half, small);
    const uint4 mask = a.mask[tile * kInstantThreads + tid];
    bf16x8 gc2[4], gc1[4], g16[2], gs1[4];
    { bf16x8 in[1] = {small}; run_step<P::step_of, P::C3t, 1>(wbase, in, nullptr, mfma, grad_epilogue(gc2, a.dzc2, mask.z, wt, col, half)); }
    run_step<P::step_of, P::C2t, 4>(wbase, gc2, nullptr, mfma, grad_epilogue(gc1, a.dzc1, mask.y, wt, col, half));
    run_step<P::step_of, P::C1t, 4>(wbase, gc1, nullptr, mfma, [&](auto, f32x16 acc) {
      if (half == 0) acc[0] += g[3];                            // row 0 of h also feeds sigma
      acc_to_operand(acc, g16[0], g16[1]);
      stash_block(a.dzs2, wt, 1, 0, col, half, g16[0], g16[1]);
    });
    { bf16x8 in[1] = {g16[0]}; run_step<P::step_of, P::S2t, 1>(wbase, in, nullptr, mfma, grad_epilogue(gs1, a.dzs1, mask.x, wt, col, half)); }
    run_step<P::step_of, P::S1t, 4>(wbase, gs1, nullptr, mfma, [&](auto, f32x16 acc) {
      if (live) feat_grad_store(a, n, half, acc, amax);
    });
  }
  // one atomic per workgroup at most, spread over kAmaxSlots words (common.h): one per wave on ONE word -- 4096 of them -- doubled
  // the Part 2 kernel's time, one per workgroup on one word still cost ~8 us of queueing at the kernel's tail
  if (a.amax_bits != nullptr) publish_amax_slots(amax, a.amax_bits);
}

}  // namespace resident
}  // namespace nerf
