// The two kernel bodies of the compiler-scheduled 8x256 decoder chain, on the blocks of mlp_chain.h.
//
//   chain_forward<P, TRAIN>   bias table, ring start, tile loop; per tile the code operand, eleven steps with the hA / hB
//                             ping-pong, the skip and view concatenations, the sigma / rgb heads; TRAIN: blocked bf16 images
//                             of every layer input and the ReLU masks [tiles][9][512]
//   chain_dgrad<OFF>          output-layer derivatives, dsmall, ten transposed steps under the stashed masks, the
//                             pre-activation gradient images
//
// Instances: mlp_fwd.hip::mlp_fwd_kernel / mlp_bwd.hip::mlp_bwd_kernel (vanilla decoder) and p3canon.hip::fwd_kernel /
// dgrad_kernel (Part 3 canonical decoder on [code(x) | code(t)]).  Each __global__ wrapper stays in its own file and
// namespace with its own argument struct; the bodies read the fields both structs have (packed, n, n_pad, rgb, sigma,
// st_*, d*), so they are templates on the argument type.  The wrapper declares the dynamic LDS array, forms tid, lane, wave,
// col and half and hands them over (formed inside the body, hipcc folded the stash addresses of the vanilla training forward
// differently and spilled eight more SGPRs); the canonical wrappers end with s_waitcnt vmcnt(0), the vanilla ones do not.
// A forward policy P supplies what differs:
//   P::Chain       the mlp_chain.h Chain (chunk and step tables, m-tile flavour)
//   P::kStreamOff  byte offsets of the forward stream and the bias table in the packed buffer
//   P::kBiasOff
//   P::Code        the code operand: kKs natural k-steps; form(a, nc, half, code, denc) makes them and the direction code
//                  of sample nc; again(half, code, out) gives the skip layer its operand (the registers of `code` again, or
//                  the code formed a second time from what the policy object kept: fewer live VGPRs, the same bits)
#pragma once
#include "mlp_chain.h"

namespace nerf {

template <class P, bool TRAIN, class Args>
__device__ __forceinline__ void chain_forward(const Args a, char* smem, int tid, int lane, int wave, int col, int half) {
  using C = typename P::Chain;
  constexpr int KC = P::Code::kKs;
  float* bias_lds = reinterpret_cast<float*>(smem);

  const float* bias_g = reinterpret_cast<const float*>(a.packed + P::kBiasOff);
  for (int i = tid; i < plan::kBiasFloats; i += kChainThreads) bias_lds[i] = bias_g[i];

  typename C::Ring ring;
  ring.init(a.packed + P::kStreamOff, smem + kBiasLdsBytes, wave, lane);
  ring.prologue();
  const char* a_base = nullptr;

  const int64_t n_tiles = (a.n + kTileSamples - 1) / kTileSamples;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const bool more = tile + gridDim.x < n_tiles;
    const int64_t n = tile * kTileSamples + wave * kWaveSamples + col;
    const bool live = n < a.n;
    const int64_t nc = live ? n : a.n - 1;

    // ---- a2 + a5: sample geometry and Fourier codes straight into MFMA B fragments ----
    typename P::Code src;
    bf16x8 code[KC], denc[2];
    src.form(a, nc, half, code, denc);
    const int64_t wave_tile = tile * 8 + wave;
    if constexpr (TRAIN) {
#pragma unroll
      for (int ks = 0; ks < KC; ++ks) stash_nat(a.st_xenc, wave_tile, KC, ks, col, half, code[ks]);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) stash_nat(a.st_denc, wave_tile, 2, ks, col, half, denc[ks]);
    }

    uint32_t mask_words[4];
    // hidden-layer epilogue: relu, bf16 operand for the next step, optional stash + mask
    auto hidden = [&](bf16x8* out, __bf16* stash, int width, bool relu) {
      return [=, &mask_words](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
        if constexpr (TRAIN) {
          if (relu) {
            uint32_t bits = 0;
#pragma unroll
            for (int r = 0; r < 16; ++r) bits |= (acc[r] > 0.0f ? 1u : 0u) << r;
            if constexpr ((m & 1) == 0) mask_words[m >> 1] = bits;
            else mask_words[m >> 1] |= bits << 16;
          }
        }
        if (relu) acc_to_operand_relu<true>(acc, out[2 * m], out[2 * m + 1]);
        else acc_to_operand_relu<false>(acc, out[2 * m], out[2 * m + 1]);
        if constexpr (TRAIN) stash_block(stash, wave_tile, width / 32, m, col, half, out[2 * m], out[2 * m + 1]);
      };
    };
    auto flush_mask = [&](int layer) {
      if constexpr (TRAIN) {
        a.st_mask[(tile * 9 + layer) * kChainThreads + tid] =
            make_uint4(mask_words[0], mask_words[1], mask_words[2], mask_words[3]);
      }
    };

    using namespace plan;
    bf16x8 hA[16], hB[16];
    // ---- a6: pts_layers.0 .. 7 (src/decoders.py:70-74) ----
    run_step<C, F_PTS0, KC, TRAIN>(ring, a_base, more, code, bias_lds, half, hidden(hA, a.st_h + 0 * a.n_pad * 256, 256, true));
    flush_mask(0);
    run_step<C, F_PTS1, 16, TRAIN>(ring, a_base, more, hA, bias_lds, half, hidden(hB, a.st_h + 1 * a.n_pad * 256, 256, true));
    flush_mask(1);
    run_step<C, F_PTS2, 16, TRAIN>(ring, a_base, more, hB, bias_lds, half, hidden(hA, a.st_h + 2 * a.n_pad * 256, 256, true));
    flush_mask(2);
    run_step<C, F_PTS3, 16, TRAIN>(ring, a_base, more, hA, bias_lds, half, hidden(hB, a.st_h + 3 * a.n_pad * 256, 256, true));
    flush_mask(3);
    {
      bf16x8 cat[16 + KC], again[KC];   // skip connection: [h3 | code], hidden first (src/decoders.py:73)
      src.again(half, code, again);
#pragma unroll
      for (int i = 0; i < 16; ++i) cat[i] = hB[i];
#pragma unroll
      for (int i = 0; i < KC; ++i) cat[16 + i] = again[i];
      run_step<C, F_PTS4, 16 + KC, TRAIN>(ring, a_base, more, cat, bias_lds, half, hidden(hA, a.st_h + 4 * a.n_pad * 256, 256, true));
      flush_mask(4);
    }
    run_step<C, F_PTS5, 16, TRAIN>(ring, a_base, more, hA, bias_lds, half, hidden(hB, a.st_h + 5 * a.n_pad * 256, 256, true));
    flush_mask(5);
    run_step<C, F_PTS6, 16, TRAIN>(ring, a_base, more, hB, bias_lds, half, hidden(hA, a.st_h + 6 * a.n_pad * 256, 256, true));
    flush_mask(6);
    run_step<C, F_PTS7, 16, TRAIN>(ring, a_base, more, hA, bias_lds, half, hidden(hB, a.st_h + 7 * a.n_pad * 256, 256, true));
    flush_mask(7);

    // ---- feature_layer (linear) + sigma_layer (relu) (src/decoders.py:77-80) ----
    {
      auto feat_epi = hidden(hA, a.st_feat, 256, false);
      run_step<C, F_HEAD, 16, TRAIN>(ring, a_base, more, hB, bias_lds, half, [&](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
        if constexpr (m < 8) feat_epi(mc, acc);
        else if (live && half == 0) a.sigma[n] = fmaxf(acc[0], 0.0f);
      });
    }
    // ---- view_layer on [feat | denc] (relu), rgb_layer (sigmoid) (src/decoders.py:83-85) ----
    {
      bf16x8 cat[18];
#pragma unroll
      for (int i = 0; i < 16; ++i) cat[i] = hA[i];
      cat[16] = denc[0];
      cat[17] = denc[1];
      mask_words[0] = mask_words[1] = mask_words[2] = mask_words[3] = 0;
      run_step<C, F_VIEW, 18, TRAIN>(ring, a_base, more, cat, bias_lds, half, hidden(hB, a.st_hv, 128, true));
      flush_mask(8);
    }
    {
      bf16x8 hv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) hv[i] = hB[i];
      run_step<C, F_RGB, 8, TRAIN>(ring, a_base, more, hv, bias_lds, half, [&](auto, f32x16 acc) {
        if (live && half == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) a.rgb[n * 3 + c] = 1.0f / (1.0f + __expf(-acc[c]));
        }
      });
    }
  }
}

// output-layer derivatives of one sample: sigmoid' and relu' applied to the upstream gradients
template <class Args>
__device__ __forceinline__ void out_derivs(const Args& a, int64_t n, float& g0, float& g1, float& g2, float& gs) {
  const float r0 = a.rgb[n * 3 + 0], r1 = a.rgb[n * 3 + 1], r2 = a.rgb[n * 3 + 2];
  g0 = a.d_rgb[n * 3 + 0] * r0 * (1.0f - r0);
  g1 = a.d_rgb[n * 3 + 1] * r1 * (1.0f - r1);
  g2 = a.d_rgb[n * 3 + 2] * r2 * (1.0f - r2);
  gs = a.sigma[n] > 0.0f ? a.d_sigma[n] : 0.0f;
}

// STREAM_OFF: byte offset of the transposed stream in the packed buffer (both decoders stream the vanilla dgrad steps:
// the code columns are never contracted)
template <size_t STREAM_OFF, class Args>
__device__ __forceinline__ void chain_dgrad(const Args a, char* smem, int tid, int lane, int wave, int col, int half) {
  using C = BwdChain;
  using namespace plan;

  C::Ring ring;
  ring.init(a.packed + STREAM_OFF, smem + kBiasLdsBytes, wave, lane);
  ring.prologue();
  const char* a_base = nullptr;

  const int64_t n_tiles = a.n_pad / kTileSamples;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const bool more = tile + gridDim.x < n_tiles;
    const int64_t wave_tile = tile * 8 + wave;
    const int64_t n = wave_tile * kWaveSamples + col;
    const bool live = n < a.n;

    // ---- output-layer derivatives: sigmoid' and relu' ----
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, gs = 0.f;
    if (live) out_derivs(a, n, g0, g1, g2, gs);
    bf16x8 small;
#pragma unroll
    for (int j = 0; j < 8; ++j) small[j] = (__bf16)0.0f;
    if (half == 0) {
      small[0] = (__bf16)g0; small[1] = (__bf16)g1; small[2] = (__bf16)g2; small[3] = (__bf16)gs;
    }
    stash_nat(a.dsmall, wave_tile, 1, 0, col, half, small);

    uint4 mask;
    auto load_mask = [&](int layer) { mask = a.st_mask[(tile * 9 + layer) * kChainThreads + tid]; };
    // epilogue: optional relu mask (bits of the layer whose output this gradient belongs to),
    // bf16 operand for the next step, blocked stash for wgrad
    auto grad_epi = [&](bf16x8* out, __bf16* stash, int width, bool masked) {
      return [=, &mask](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
        if (masked) {
          const uint32_t words[4] = {mask.x, mask.y, mask.z, mask.w};
          const uint32_t bits = words[m >> 1] >> (16 * (m & 1));
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = (bits >> r) & 1u ? acc[r] : 0.0f;
        }
        acc_to_operand(acc, out[2 * m], out[2 * m + 1]);
        stash_block(stash, wave_tile, width / 32, m, col, half, out[2 * m], out[2 * m + 1]);
      };
    };

    bf16x8 gA[16], gB[16];
    // ---- rgb_layer^T: d(hv_pre) = relu'(hv) * W_rgb^T d(rgb_pre) ----
    {
      bf16x8 in[1];
      in[0] = small;
      if (half == 0) in[0][3] = (__bf16)0.0f;   // column 3 carries d(sigma_pre), not an rgb row
      load_mask(8);
      run_step<C, B_RGB, 1, true>(ring, a_base, more, in, nullptr, half, grad_epi(gA, a.dhv, 128, true));
    }
    // ---- view_layer^T (feature columns only): d(feat) ----
    {
      bf16x8 in[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) in[i] = gA[i];
      run_step<C, B_VIEW, 8, true>(ring, a_base, more, in, nullptr, half, grad_epi(gB, a.dfeat, 256, false));
    }
    // ---- (feature_layer | sigma_layer)^T: d(h7_pre) ----
    {
      bf16x8 in[17];
#pragma unroll
      for (int i = 0; i < 16; ++i) in[i] = gB[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) in[16][j] = (__bf16)0.0f;
      if (half == 0) in[16][0] = (__bf16)gs;
      load_mask(7);
      run_step<C, B_HEAD, 17, true>(ring, a_base, more, in, nullptr, half, grad_epi(gA, a.dh + 7 * a.n_pad * 256, 256, true));
    }
    // ---- pts_layers.7 .. 1 transposed: d(h_{l-1}_pre) ----
    load_mask(6);
    run_step<C, B_PTS7, 16, true>(ring, a_base, more, gA, nullptr, half, grad_epi(gB, a.dh + 6 * a.n_pad * 256, 256, true));
    load_mask(5);
    run_step<C, B_PTS6, 16, true>(ring, a_base, more, gB, nullptr, half, grad_epi(gA, a.dh + 5 * a.n_pad * 256, 256, true));
    load_mask(4);
    run_step<C, B_PTS5, 16, true>(ring, a_base, more, gA, nullptr, half, grad_epi(gB, a.dh + 4 * a.n_pad * 256, 256, true));
    load_mask(3);
    run_step<C, B_PTS4, 16, true>(ring, a_base, more, gB, nullptr, half, grad_epi(gA, a.dh + 3 * a.n_pad * 256, 256, true));
    load_mask(2);
    run_step<C, B_PTS3, 16, true>(ring, a_base, more, gA, nullptr, half, grad_epi(gB, a.dh + 2 * a.n_pad * 256, 256, true));
    load_mask(1);
    run_step<C, B_PTS2, 16, true>(ring, a_base, more, gB, nullptr, half, grad_epi(gA, a.dh + 1 * a.n_pad * 256, 256, true));
    load_mask(0);
    run_step<C, B_PTS1, 16, true>(ring, a_base, more, gA, nullptr, half, grad_epi(gB, a.dh + 0 * a.n_pad * 256, 256, true));
  }
}

}  // namespace nerf
