// Part 3 canonical decoder on the fused 8x256 chain: NeRFDecoder on [code(x) | code(t)] (reference src/core.py:108-113 and
// 233-281, src/decoders.py:29-87) for `canonical_type: nerf` (code(x_c) L 10, code(t') L 10: 84 columns) and for
// `direct_time_conditioning` (code(x) L 10, code(t) L <= 10).  Plan: p3canon_plan.h.
//
//   fwd_kernel     the vanilla forward chain (mlp_fwd.hip, compiler-scheduled family) with six natural code k-steps at
//                  pts_layers.0 and at the skip; the codes are formed in registers from x [n,3] and t [n] (and formed
//                  again at the skip instead of being held live through layers 0..3).  TRAIN: blocked bf16 images of
//                  every layer input and the ReLU masks, as the vanilla forward writes them.
//   dgrad_kernel   the vanilla transposed chain (mlp_bwd.hip) on this layout's dgrad stream: pre-activation gradient images.
//   dcode_kernel   d code(x) = W0[:, :63]^T dz0 + W4[:, 256:319]^T dz4 from the bf16 images of dz0 / dz4, then the Fourier
//                  chain rule to d x [n,3], ADDED to the caller's vector (x_c = x + delta_x).
//   weight grads   mlp_wgrad.hip's split-K kernel with this decoder's job table (partial tiles + ordered reduction into a
//                  gradient image of fixed layout), then remap_kernel into the reference layout.
#include <stddef.h>
#include <stdint.h>
#include "mlp_chain.h"
#include "mlp_stash.h"
#include "mlp_wgrad.h"
#include "p3canon_plan.h"

namespace nerf {
namespace p3c {
using plan::Chunks;
using plan::Step;

// ---------------------------------------------------------------------------------------------------- forward weight ring
// mlp_chain.h::WeightRing<false> over this plan's chunk table
struct CanonRing {
  static constexpr const Chunks& chunks() { return cplan::kFwdChunks; }
  const char* stream;
  char* lds;
  int slot;
  int wave, lane;

  __device__ __forceinline__ void init(const char* s, char* l, int w, int ln) {
    stream = s; lds = l; slot = 1; wave = w; lane = ln;
  }
  template <int C>
  __device__ __forceinline__ void issue(int dst_slot) const {
    constexpr int frag0 = chunks().chunk_frag0[C];
    constexpr int count = chunks().chunk_count[C];
    const char* sbase = stream;
    asm volatile("" : "+s"(sbase));
    sbase += (size_t)(frag0 + wave) * 1024;
    char* dst = lds + dst_slot * kRingSlotBytes + wave * 1024;
    const uint32_t voff = (uint32_t)lane * 16u;
#pragma unroll
    for (int i = 0; i < (count + 7) / 8; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(sbase + i * 8192 + voff), (lptr_t)(dst + i * 8192), 16, 0, 0);
  }
  __device__ __forceinline__ void prologue() { issue<0>(0); }
  template <int C, int STORES>
  __device__ __forceinline__ const char* advance(bool more_passes) {
    constexpr int n = chunks().n_chunks;
    static_assert(STORES >= 0 && STORES < 48, "vmcnt immediate");
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(STORES) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    slot ^= 1;
    if constexpr (C + 1 < n) issue<C + 1>(slot ^ 1);
    else if (more_passes) issue<0>(slot ^ 1);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    return lds + slot * kRingSlotBytes + lane * 16;
  }
};

// stash stores issued while the chunk before the one group g opens was consumed (under-counting is safe: see WeightRing)
constexpr int prev_chunk_stores(int g) {
  const Chunks& ch = cplan::kFwdChunks;
  const int c = ch.group_chunk[g];
  if (c == 0) return 0;
  int n = 0;
  for (int i = 0; i < ch.n_groups; ++i) n += ch.group_chunk[i] == c - 1 ? group_stores<false>(i) : 0;   // same m-tiles per step as vanilla
  return n < 47 ? n : 47;
}

template <int KIND, int KS, bool STASH, class Epi>
__device__ __forceinline__ void fwd_step(CanonRing& ring, const char*& a_base, bool more_passes, const bf16x8 (&b)[KS],
                                         const float* bias_lds, int half, Epi&& epi) {
  constexpr Step st = cplan::step_of(KIND);
  static_assert(KS == st.ks_acc + st.ks_nat, "operand k-steps");
  static_for<st.mt>([&](auto mc) {
    constexpr int m = decltype(mc)::value;
    constexpr int g = cplan::group_of(KIND, m);
    constexpr const Chunks& ch = cplan::kFwdChunks;
    if constexpr (ch.group_first[g])
      a_base = ring.template advance<ch.group_chunk[g], STASH ? prev_chunk_stores(g) : 0>(more_passes);
    f32x16 acc = bias_tile(bias_lds, plan::bias_off(KIND) + 32 * m, half);
    acc = mtile<KS>(a_base, ch.group_off[g], b, acc);
    epi(mc, acc);
  });
}

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
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
  s.xenc = take(np * cplan::kCodeK * 2);
  s.h = take(np * 256 * 2 * 8);
  s.feat = take(np * 256 * 2);
  s.hv = take(np * 128 * 2);
  s.denc = take(np * 32 * 2);
  s.mask = take((np / 256) * 9 * 512 * 16);
  s.dsmall = take(np * 16 * 2);
  s.dhv = take(np * 128 * 2);
  s.dfeat = take(np * 256 * 2);
  s.dh = take(np * 256 * 2 * 8);
  s.egrad = take((size_t)cplan::eCount * 4);
  s.slab_bytes = slab_bytes(n);
  s.slab = take(s.slab_bytes);
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

template <bool TRAIN>
__global__ void __launch_bounds__(kChainThreads, 2) fwd_kernel(const FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* bias_lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, half = lane >> 5;

  const float* bias_g = reinterpret_cast<const float*>(a.packed + cplan::kPackBiasOff);
  for (int i = tid; i < plan::kBiasFloats; i += kChainThreads) bias_lds[i] = bias_g[i];

  CanonRing ring;
  ring.init(a.packed + cplan::kPackFwdOff, smem + kBiasLdsBytes, wave, lane);
  ring.prologue();
  const char* a_base = nullptr;

  const int64_t n_tiles = (a.n + kTileSamples - 1) / kTileSamples;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const bool more = tile + gridDim.x < n_tiles;
    const int64_t n = tile * kTileSamples + wave * kWaveSamples + col;
    const bool live = n < a.n;
    const int64_t nc = live ? n : a.n - 1;
    const float px = a.x[nc * 3 + 0], py = a.x[nc * 3 + 1], pz = a.x[nc * 3 + 2], tt = a.t[nc];
    const int64_t wave_tile = tile * 8 + wave;

    bf16x8 code[cplan::kCodeKs];
    code_operand(px, py, pz, tt, half, code);
    bf16x8 denc[2];
    fourier_operand<2, plan::kDirDim>(a.dirs[nc * 3 + 0], a.dirs[nc * 3 + 1], a.dirs[nc * 3 + 2], half, denc);
    if constexpr (TRAIN) {
#pragma unroll
      for (int ks = 0; ks < cplan::kCodeKs; ++ks) stash_nat(a.st_xenc, wave_tile, cplan::kCodeKs, ks, col, half, code[ks]);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) stash_nat(a.st_denc, wave_tile, 2, ks, col, half, denc[ks]);
    }

    uint32_t mask_words[4];
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
      if constexpr (TRAIN)
        a.st_mask[(tile * 9 + layer) * kChainThreads + tid] = make_uint4(mask_words[0], mask_words[1], mask_words[2], mask_words[3]);
    };

    bf16x8 hA[16], hB[16];
    // pts_layers.0 .. 3 on the code (src/decoders.py:70-74)
    fwd_step<plan::F_PTS0, 6, TRAIN>(ring, a_base, more, code, bias_lds, half, hidden(hA, a.st_h + 0 * a.n_pad * 256, 256, true));
    flush_mask(0);
    fwd_step<plan::F_PTS1, 16, TRAIN>(ring, a_base, more, hA, bias_lds, half, hidden(hB, a.st_h + 1 * a.n_pad * 256, 256, true));
    flush_mask(1);
    fwd_step<plan::F_PTS2, 16, TRAIN>(ring, a_base, more, hB, bias_lds, half, hidden(hA, a.st_h + 2 * a.n_pad * 256, 256, true));
    flush_mask(2);
    fwd_step<plan::F_PTS3, 16, TRAIN>(ring, a_base, more, hA, bias_lds, half, hidden(hB, a.st_h + 3 * a.n_pad * 256, 256, true));
    flush_mask(3);
    {
      // skip connection [h3 | code], hidden first (src/decoders.py:73); the code is formed again from x, t: the same
      // arithmetic on the same values (the same bits), 20 VGPRs fewer live through layers 0..3
      bf16x8 cat[22], again[cplan::kCodeKs];
      code_operand(px, py, pz, tt, half, again);
#pragma unroll
      for (int i = 0; i < 16; ++i) cat[i] = hB[i];
#pragma unroll
      for (int i = 0; i < cplan::kCodeKs; ++i) cat[16 + i] = again[i];
      fwd_step<plan::F_PTS4, 22, TRAIN>(ring, a_base, more, cat, bias_lds, half, hidden(hA, a.st_h + 4 * a.n_pad * 256, 256, true));
      flush_mask(4);
    }
    fwd_step<plan::F_PTS5, 16, TRAIN>(ring, a_base, more, hA, bias_lds, half, hidden(hB, a.st_h + 5 * a.n_pad * 256, 256, true));
    flush_mask(5);
    fwd_step<plan::F_PTS6, 16, TRAIN>(ring, a_base, more, hB, bias_lds, half, hidden(hA, a.st_h + 6 * a.n_pad * 256, 256, true));
    flush_mask(6);
    fwd_step<plan::F_PTS7, 16, TRAIN>(ring, a_base, more, hA, bias_lds, half, hidden(hB, a.st_h + 7 * a.n_pad * 256, 256, true));
    flush_mask(7);
    // feature_layer (linear) + sigma_layer (relu) (src/decoders.py:77-80)
    {
      auto feat_epi = hidden(hA, a.st_feat, 256, false);
      fwd_step<plan::F_HEAD, 16, TRAIN>(ring, a_base, more, hB, bias_lds, half, [&](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
        if constexpr (m < 8) feat_epi(mc, acc);
        else if (live && half == 0) a.sigma[n] = fmaxf(acc[0], 0.0f);
      });
    }
    // view_layer on [feat | denc] (relu), rgb_layer (sigmoid) (src/decoders.py:83-85)
    {
      bf16x8 cat[18];
#pragma unroll
      for (int i = 0; i < 16; ++i) cat[i] = hA[i];
      cat[16] = denc[0];
      cat[17] = denc[1];
      mask_words[0] = mask_words[1] = mask_words[2] = mask_words[3] = 0;
      fwd_step<plan::F_VIEW, 18, TRAIN>(ring, a_base, more, cat, bias_lds, half, hidden(hB, a.st_hv, 128, true));
      flush_mask(8);
    }
    {
      bf16x8 hv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) hv[i] = hB[i];
      fwd_step<plan::F_RGB, 8, TRAIN>(ring, a_base, more, hv, bias_lds, half, [&](auto, f32x16 acc) {
        if (live && half == 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) a.rgb[n * 3 + c] = 1.0f / (1.0f + __expf(-acc[c]));
        }
      });
    }
  }
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

// mlp_bwd.hip::mlp_bwd_kernel on this layout's transposed stream (the same steps: the code columns are never contracted)
__global__ void __launch_bounds__(kChainThreads, 2) dgrad_kernel(const BwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, half = lane >> 5;

  WeightRing<true> ring;
  ring.init(a.packed + cplan::kPackBwdOff, smem + kBiasLdsBytes, wave, lane);
  ring.prologue();
  const char* a_base = nullptr;

  const int64_t n_tiles = a.n_pad / kTileSamples;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const bool more = tile + gridDim.x < n_tiles;
    const int64_t wave_tile = tile * 8 + wave;
    const int64_t n = wave_tile * kWaveSamples + col;
    const bool live = n < a.n;

    // output-layer derivatives: sigmoid' and relu'
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, gs = 0.f;
    if (live) {
      const float r0 = a.rgb[n * 3 + 0], r1 = a.rgb[n * 3 + 1], r2 = a.rgb[n * 3 + 2];
      g0 = a.d_rgb[n * 3 + 0] * r0 * (1.0f - r0);
      g1 = a.d_rgb[n * 3 + 1] * r1 * (1.0f - r1);
      g2 = a.d_rgb[n * 3 + 2] * r2 * (1.0f - r2);
      gs = a.sigma[n] > 0.0f ? a.d_sigma[n] : 0.0f;
    }
    bf16x8 small;
#pragma unroll
    for (int j = 0; j < 8; ++j) small[j] = (__bf16)0.0f;
    if (half == 0) {
      small[0] = (__bf16)g0; small[1] = (__bf16)g1; small[2] = (__bf16)g2; small[3] = (__bf16)gs;
    }
    stash_nat(a.dsmall, wave_tile, 1, 0, col, half, small);

    uint4 mask;
    auto load_mask = [&](int layer) { mask = a.st_mask[(tile * 9 + layer) * kChainThreads + tid]; };
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
    {
      bf16x8 in[1];
      in[0] = small;
      if (half == 0) in[0][3] = (__bf16)0.0f;   // column 3 carries d(sigma_pre), not an rgb row
      load_mask(8);
      run_step<true, plan::B_RGB, 1, true>(ring, a_base, more, in, nullptr, half, grad_epi(gA, a.dhv, 128, true));
    }
    {
      bf16x8 in[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) in[i] = gA[i];
      run_step<true, plan::B_VIEW, 8, true>(ring, a_base, more, in, nullptr, half, grad_epi(gB, a.dfeat, 256, false));
    }
    {
      bf16x8 in[17];
#pragma unroll
      for (int i = 0; i < 16; ++i) in[i] = gB[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) in[16][j] = (__bf16)0.0f;
      if (half == 0) in[16][0] = (__bf16)gs;
      load_mask(7);
      run_step<true, plan::B_HEAD, 17, true>(ring, a_base, more, in, nullptr, half, grad_epi(gA, a.dh + 7 * a.n_pad * 256, 256, true));
    }
    load_mask(6);
    run_step<true, plan::B_PTS7, 16, true>(ring, a_base, more, gA, nullptr, half, grad_epi(gB, a.dh + 6 * a.n_pad * 256, 256, true));
    load_mask(5);
    run_step<true, plan::B_PTS6, 16, true>(ring, a_base, more, gB, nullptr, half, grad_epi(gA, a.dh + 5 * a.n_pad * 256, 256, true));
    load_mask(4);
    run_step<true, plan::B_PTS5, 16, true>(ring, a_base, more, gA, nullptr, half, grad_epi(gB, a.dh + 4 * a.n_pad * 256, 256, true));
    load_mask(3);
    run_step<true, plan::B_PTS4, 16, true>(ring, a_base, more, gB, nullptr, half, grad_epi(gA, a.dh + 3 * a.n_pad * 256, 256, true));
    load_mask(2);
    run_step<true, plan::B_PTS3, 16, true>(ring, a_base, more, gA, nullptr, half, grad_epi(gB, a.dh + 2 * a.n_pad * 256, 256, true));
    load_mask(1);
    run_step<true, plan::B_PTS2, 16, true>(ring, a_base, more, gB, nullptr, half, grad_epi(gA, a.dh + 1 * a.n_pad * 256, 256, true));
    load_mask(0);
    run_step<true, plan::B_PTS1, 16, true>(ring, a_base, more, gA, nullptr, half, grad_epi(gB, a.dh + 0 * a.n_pad * 256, 256, true));
  }
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
      for (int k = 0; k < cplan::step_ks(kind); ++k) t.v[f++] = (kind << 16) | (m << 8) | k;
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
      const int k = nat ? 16 * (ks - st.ks_acc) + 8 * h + j : 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
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

int grid_for(int64_t tiles) {
  int n_cu = 0;
  if (device_cu_count(&n_cu) != NERF_OK) return -1;
  return (int)(tiles < n_cu ? tiles : n_cu);
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
  const int grid = p3c::grid_for(l.n_pad / kTileSamples);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p3_canon_fwd: cannot query device");
  const void* kernel = train ? (const void*)p3c::fwd_kernel<true> : (const void*)p3c::fwd_kernel<false>;
  if (int rc = ensure_dynamic_lds(kernel, kChainLds, "nerf_p3_canon_fwd"); rc != NERF_OK) return rc;
  if (train) hipLaunchKernelGGL(p3c::fwd_kernel<true>, dim3(grid), dim3(kChainThreads), kChainLds, as_stream(stream), a);
  else hipLaunchKernelGGL(p3c::fwd_kernel<false>, dim3(grid), dim3(kChainThreads), kChainLds, as_stream(stream), a);
  return check_launch("nerf_p3_canon_fwd");
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
  const int grid = p3c::grid_for(l.n_pad / kTileSamples);
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
