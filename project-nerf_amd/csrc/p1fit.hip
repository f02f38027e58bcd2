// Part 1 image fit (reference run.py:30-237 with NeuralField('part1_fourier'), src/core.py:25-34, src/embeddings.py:22-32,
// src/decoders.py:6-26) as a fused register chain with its loss, backward and weight gradients:
//
//   code = [x | sin(2^0 pi x) | cos(2^0 pi x) | ...]     2 + 4 L columns (L = 0 or use_positional_encoding false: the 2 raw ones)
//   h_1  = relu(W_1 code + b_1)                          -> H
//   h_i  = relu(W_i h_{i-1} + b_i)    i = 2..layers      H -> H
//   y    = sigmoid(W_out h_last + b_out)                 H -> 3
//   loss = mean((y - target)^2)                          over n * 3 values
//
// Compiled: H in {64, 128, 256}, 1..8 layers, L 0..15.  The sample-major register chain of sample_chain.h (staging, tile loop, image
// rows, the weight-gradient job and the host helpers live there): 32 samples per wave on the MFMA column
// (v_mfma_f32_32x32x16_bf16), accumulator tiles -> bf16 B fragments of the next layer, 8 waves (256 samples) per workgroup pass.
// All hidden layers have one shape, so the chain is a runtime loop over layers for a templated H.
//
// Where the weights live: ONE layer at a time is staged from the packed fragment image (L2) into LDS, for every H (H = 256: one
// layer is 128 KiB of the 160; H = 64 / 128 could keep several resident, the one code path was preferred).  Biases initialise
// the accumulators, read from the packed image.
//
// Layer-1 operand, 64 columns: [x_hi y_hi | x_lo y_lo | sin/cos columns (4 L) | 0 ...].  x_hi = bf16(x), x_lo = bf16(x - x_hi),
// both contracted against the same weight column: the raw coordinates keep >= 16 significant bits (adjacent pixels of a 400-wide
// image are 2.5e-3 apart, one bf16 step in [0.5, 1) is 1.95e-3).  The trigonometric columns are single bf16; their argument is
// (x * 2^band) * pi with both products rounded to fp32 and full-range sinf / cosf, the arithmetic of fourier.hip (arguments reach
// 2^14 pi: outside the hardware sine's range).
//
// Training images are row-major bf16: code [n_pad][64] (operand columns), h_1..h_last and dz_1..dz_last [n_pad][H], d_pre
// [n_pad][8]; the relu masks are h > 0 of the stored values.  The training forward fuses sigmoid + MSE + their derivative
// d_pre = 2/(3n) (y - t) y (1 - y) and writes one partial loss per workgroup, added in workgroup order by the reduction launch.
// The dgrad kernel runs the transposed chain on the stored masks (no input gradient: coordinates are not learned).  Weight and bias
// gradients: chunk-partial tiles over the sample axis on bf16 MFMA (samples on the k axis, images transposed through LDS), then
// one reduction in chunk order.  No float atomics anywhere: the same bits on every run.
//
// tools/kernel_resources.py (VGPRs; scratch 0 and no spills in every kernel): fwd_kernel<64 / 128 / 256> training 100 / 130 / 256,
// inference 91 / 135 / 256 + 114 AGPRs -- at H = 256 the two 64-register operand arrays and the row index do not fit 256 registers,
// so that instance runs 4 waves per workgroup; dgrad_kernel<64 / 128 / 256> 70 / 106 / 239; wgrad_kernel 72 + 64 AGPRs.
//
// Parameter vector (fp32, the module's state dict concatenated, [out, in] row-major): decoder.net.{0,2,...}.{weight,bias}
//   W_1 [H, C] b_1 [H] | W_i [H, H] b_i [H] (i = 2..layers) | W_out [3, H] b_out [3]          C = 2 + 4 L
#include <math.h>
#include "sample_chain.h"

namespace nerf {
namespace p1 {
using namespace sample_chain;

constexpr int kThreads = 512, kWaves = kThreads / 64, kTile = kWaves * 32;
constexpr int kCodeLd = 64, kCodeKs = kCodeLd / 16, kDpreLd = 8;
constexpr int kMaxLayers = 8, kMaxL = 15;
constexpr int kLossParts = 4096;

// fragment plan (1-KiB fragments) and parameter offsets of one shape
struct Plan {
  int H, layers, L, C, mt, ks;
  int f1, hid0, out, bout_t, hid_t0, frags;      // first fragment of: layer 1, hidden 2.., output, output^T, hidden^T 2..
  int n_params, slab_stride;                     // slab row: the parameter vector + W_1 by operand column [H][64]
  __host__ __device__ int w_off(int l) const { return l == 0 ? 0 : H * C + H + (l - 1) * (H * H + H); }   // l = layers: W_out
  __host__ __device__ int b_off(int l) const { return w_off(l) + (l == 0 ? H * C : (l == layers ? 3 * H : H * H)); }
  __host__ __device__ size_t bias_bytes_off() const { return (size_t)frags * 1024; }
};
static bool make_plan(int L, int use_pe, int H, int layers, Plan* p) {
  if (!(H == 64 || H == 128 || H == 256) || layers < 1 || layers > kMaxLayers || L < 0 || L > kMaxL) return false;
  p->H = H; p->layers = layers; p->L = use_pe ? L : 0; p->C = 2 + 4 * p->L; p->mt = H / 32; p->ks = H / 16;
  const int per = p->mt * p->ks;
  p->f1 = 0; p->hid0 = p->mt * kCodeKs; p->out = p->hid0 + (layers - 1) * per; p->bout_t = p->out + p->ks;
  p->hid_t0 = p->bout_t + p->mt; p->frags = p->hid_t0 + (layers - 1) * per;
  p->n_params = p->b_off(layers) + 3;
  p->slab_stride = p->n_params + H * kCodeLd;
  return true;
}
static size_t packed_bytes(const Plan& p) { return p.bias_bytes_off() + (size_t)(p.layers * p.H + 32) * 4; }

__global__ void __launch_bounds__(256) pack_kernel(const float* __restrict__ params, char* __restrict__ packed, const Plan p) {
  const int per = p.mt * p.ks;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < p.frags * 64; t += gridDim.x * blockDim.x) {
    const int frag = t >> 6, lane = t & 63, h = lane >> 5;
    enum { F1, HID, OUT, BOUT, HIDT } step;
    int rel, layer = 0, mt = 0, ks = 0;
    if (frag < p.hid0) { step = F1; rel = frag; mt = rel / kCodeKs; ks = rel % kCodeKs; }
    else if (frag < p.out) { step = HID; rel = frag - p.hid0; layer = 1 + rel / per; mt = rel % per / p.ks; ks = rel % p.ks; }
    else if (frag < p.bout_t) { step = OUT; ks = frag - p.out; }
    else if (frag < p.hid_t0) { step = BOUT; mt = frag - p.bout_t; }
    else { step = HIDT; rel = frag - p.hid_t0; layer = 1 + rel / per; mt = rel % per / p.ks; ks = rel % p.ks; }
    const bool nat = step == F1 || step == BOUT;
    const int row = mt * 32 + (lane & 31);
    unsigned short out[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = frag_column(ks, h, j, nat);
      int src = -1;
      switch (step) {
        case F1: {       // operand columns [x_hi y_hi | x_lo y_lo | code columns 2..C-1]
          const int c = k < 2 ? k : k - 2;
          if (c < p.C) src = row * p.C + c;
          break;
        }
        case HID: src = p.w_off(layer) + row * p.H + k; break;
        case OUT: if (row < 3) src = p.w_off(p.layers) + row * p.H + k; break;
        case BOUT: if (k < 3) src = p.w_off(p.layers) + k * p.H + row; break;
        default: src = p.w_off(layer) + k * p.H + row; break;
      }
      out[j] = __builtin_bit_cast(unsigned short, (__bf16)(src >= 0 ? params[src] : 0.0f));
    }
    store_fragment(packed, frag, lane, out);
  }
  if (blockIdx.x == 0) {
    float* bias = reinterpret_cast<float*>(packed + p.bias_bytes_off());        // b_1 .. b_layers [H] each | b_out padded to 32
    const int nb = p.layers * p.H;
    for (int i = threadIdx.x; i < nb + 32; i += blockDim.x)
      bias[i] = i < nb ? params[p.b_off(i / p.H) + i % p.H] : (i - nb < 3 ? params[p.b_off(p.layers) + i - nb] : 0.0f);
  }
}

struct Args {
  const char* packed;
  Plan p;
  const float* coords;       // [N,2]
  const int64_t* idx;        // [n] rows of coords / target, or NULL: rows 0..n
  const float* target;       // [N,3]
  int64_t n, n_pad;
  float dscale;              // 2 / (3 n)
  float* y;                  // [n,3] (inference)
  float* loss_part;          // one squared-error sum per workgroup
  __bf16* code; __bf16* h; __bf16* dz; __bf16* dpre;     // training images; h / dz: [layers][n_pad][H]
};

// H = 256 holds two 64-register operand arrays and reads 2 fragments ahead (a depth of 3 spilled three registers)
constexpr int ahead(int H) { return H == 256 ? 2 : kAhead; }
// inference at H = 256 runs 4 waves per workgroup: two 64-register operand arrays + the row index did not fit 256 registers
constexpr int fwd_waves(int H, bool train) { return (!train && H == 256) ? 4 : kWaves; }
template <int H, bool TRAIN>
__global__ void __launch_bounds__((64 * fwd_waves(H, TRAIN))) fwd_kernel(const Args a) {
  constexpr int MT = H / 32, KS = H / 16, WAVES = fwd_waves(H, TRAIN), AH = ahead(H);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = smem + lane * 16;
  const float* bias = reinterpret_cast<const float*>(a.packed + a.p.bias_bytes_off());
  const int layers = a.p.layers, L = a.p.L;
  const int64_t n_tiles = a.n_pad / (WAVES * 32);
  const size_t img = (size_t)a.n_pad * H;
  float lsum = 0.0f;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t n = (tile * WAVES + wave) * 32 + col;
    const bool live = n < a.n;
    const int64_t nc = live ? n : a.n - 1;
    const int64_t r = a.idx != nullptr ? a.idx[nc] : nc;
    const float x0 = a.coords[r * 2 + 0], x1 = a.coords[r * 2 + 1];
    // layer-1 operand, natural order: column f = 16 ks + 8 half + j.  f < 4: the raw pair as hi / lo; else code column
    // f - 2, i.e. band (f - 4) / 4, axis j & 1, cosine iff j & 2 (f - 4 and j agree modulo 4)
    bf16x8 code[kCodeKs];
#pragma unroll
    for (int ks = 0; ks < kCodeKs; ++ks) {
      bf16x8 cb;
#pragma unroll
      for (int j = 0; j < 8; ++j) cb[j] = (__bf16)0.0f;
      if (16 * ks < 4 + 4 * L) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int band = 4 * ks + 2 * half + (j >> 2) - 1;
          const bool raw = band < 0;
          const float xa = (j & 1) ? x1 : x0;
          // trig: (x * 2^band) * pi, both products rounded to fp32 (src/embeddings.py:30-31)
          float v = 0.0f;
          if (raw) v = (j & 2) ? xa - (float)(__bf16)xa : xa;
          else if (band < L) {       // bands past L cost no sine
            const float arg = mul_rn(mul_rn(xa, (float)(1u << band)), 3.14159265358979323846f);
            v = (j & 2) ? cosf(arg) : sinf(arg);
          }
          cb[j] = (__bf16)v;
        }
      }
      code[ks] = cb;
      __builtin_amdgcn_sched_barrier(0);       // one k-step's eight sines at a time
      if constexpr (TRAIN) *reinterpret_cast<bf16x8*>(a.code + n * kCodeLd + 16 * ks + 8 * half) = cb;
    }
    auto relu_epi = [&](bf16x8* out, __bf16* himg) {
      return [=](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
        acc_to_operand_relu<true>(acc, out[2 * m], out[2 * m + 1]);
        if constexpr (TRAIN) store_rows(himg, H, n, m, half, out[2 * m], out[2 * m + 1]);
      };
    };
    bf16x8 hc[KS];
    stage<WAVES>(smem, a.packed + (size_t)a.p.f1 * 1024, MT * kCodeKs);
    run<0, MT, kCodeKs, AH>(wbase, code, bias, half, relu_epi(hc, a.h));
#pragma unroll 1
    for (int l = 1; l < layers; ++l) {
      stage<WAVES>(smem, a.packed + ((size_t)a.p.hid0 + (size_t)(l - 1) * MT * KS) * 1024, MT * KS);
      bf16x8 hn[KS];
      run<0, MT, KS, AH>(wbase, hc, bias + l * H, half, relu_epi(hn, a.h + l * img));
#pragma unroll
      for (int k = 0; k < KS; ++k) hc[k] = hn[k];
    }
    stage<WAVES>(smem, a.packed + (size_t)a.p.out * 1024, KS);
    auto out_epi = [&](auto, f32x16 acc) {
      if (half != 0) return;
      bf16x8 d;
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = (__bf16)0.0f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float z = acc[c] + bias[layers * H + c];
        const float y = 1.0f / (1.0f + expf(-z));
        if constexpr (TRAIN) {
          if (live) {
            const float e = y - a.target[r * 3 + c];
            lsum = __builtin_fmaf(e, e, lsum);
            d[c] = (__bf16)(a.dscale * e * y * (1.0f - y));
          }
        } else {
          if (live) a.y[n * 3 + c] = y;
        }
      }
      if constexpr (TRAIN) *reinterpret_cast<bf16x8*>(a.dpre + n * kDpreLd) = d;
    };
    run<0, 1, KS, kAhead>(wbase, hc, nullptr, half, out_epi);
  }
  if constexpr (TRAIN) {
    // this workgroup's squared-error sum: lanes by butterfly, waves in wave order
    float* part = reinterpret_cast<float*>(smem);
    lsum = wave_sum(lsum);
    __syncthreads();
    if (lane == 0) part[wave] = lsum;
    __syncthreads();
    if (tid == 0) {
      float s = 0.0f;
      for (int w = 0; w < WAVES; ++w) s += part[w];
      a.loss_part[blockIdx.x] = s;
    }
  }
}

template <int H>
__global__ void __launch_bounds__(kThreads) dgrad_kernel(const Args a) {
  constexpr int MT = H / 32, KS = H / 16, AH = ahead(H);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = smem + lane * 16;
  const int layers = a.p.layers;
  const int64_t n_tiles = a.n_pad / kTile;
  const size_t img = (size_t)a.n_pad * H;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t n = (tile * kWaves + wave) * 32 + col;
    bf16x8 small[1];
#pragma unroll
    for (int j = 0; j < 8; ++j) small[0][j] = (__bf16)0.0f;
    if (half == 0) small[0] = *reinterpret_cast<const bf16x8*>(a.dpre + n * kDpreLd);       // zero beyond n (forward)
    // d h_k -> dz_k = d h_k [h_k > 0] (stored activations): bf16 operand of the next transposed layer + image for the wgrad
    auto mask_epi = [&](bf16x8* out, const __bf16* h, __bf16* dz) {
      return [=](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
        float hv[16];
        load_rows(h, H, n, m, half, hv);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = hv[r] > 0.0f ? acc[r] : 0.0f;
        acc_to_operand(acc, out[2 * m], out[2 * m + 1]);
        store_rows(dz, H, n, m, half, out[2 * m], out[2 * m + 1]);
      };
    };
    bf16x8 g[KS];
    stage<kWaves>(smem, a.packed + (size_t)a.p.bout_t * 1024, MT);
    run<0, MT, 1, AH>(wbase, small, nullptr, half, mask_epi(g, a.h + (layers - 1) * img, a.dz + (layers - 1) * img));
#pragma unroll 1
    for (int l = layers - 1; l >= 1; --l) {
      stage<kWaves>(smem, a.packed + ((size_t)a.p.hid_t0 + (size_t)(l - 1) * MT * KS) * 1024, MT * KS);
      bf16x8 gn[KS];
      run<0, MT, KS, AH>(wbase, g, nullptr, half, mask_epi(gn, a.h + (l - 1) * img, a.dz + (l - 1) * img));
#pragma unroll
      for (int k = 0; k < KS; ++k) g[k] = gn[k];
    }
  }
}

// Weight gradients (sample_chain.h::wgrad_job).  blockIdx.x: chunk, blockIdx.y: job = layer * (H / 64) + block, last job: the
// output layer.  Layer 1 contracts against the operand columns [H][64], kept after the parameter vector in the slab row.
struct WgradArgs {
  Plan p;
  const __bf16* code; const __bf16* h; const __bf16* dz; const __bf16* dpre;
  int64_t n, n_pad, chunk;
  float* slab;               // [chunks][slab_stride]
};
__device__ __forceinline__ Job job_of(const WgradArgs& a, int job) {
  const Plan& p = a.p;
  const int H = p.H, blocks = H / kOBlock;
  const size_t img = (size_t)a.n_pad * H;
  Job j{};
  if (job == p.layers * blocks) {
    j.A = a.dpre; j.a_ld = kDpreLd; j.O = 3; j.o0 = 0;
    j.B = a.h + (p.layers - 1) * img; j.b_ld = H; j.I = H;
    j.w_off = p.w_off(p.layers); j.w_ld = H; j.b_off = p.b_off(p.layers);
  } else {
    const int l = job / blocks;
    j.A = a.dz + l * img; j.a_ld = H; j.O = H; j.o0 = (job % blocks) * kOBlock;
    j.B = l == 0 ? a.code : a.h + (l - 1) * img; j.b_ld = l == 0 ? kCodeLd : H; j.I = j.b_ld;
    j.w_off = l == 0 ? p.n_params : p.w_off(l); j.w_ld = j.I; j.b_off = p.b_off(l);
  }
  return j;
}
__global__ void __launch_bounds__(256) wgrad_kernel(const WgradArgs a) {
  const Job jb = job_of(a, blockIdx.y);
  const int64_t n0 = blockIdx.x * a.chunk;
  const int64_t n1 = n0 + a.chunk < a.n ? n0 + a.chunk : a.n;
  wgrad_job(jb, n0, n1, a.slab + (size_t)blockIdx.x * a.p.slab_stride);
}

// grads[q] = sum over chunks, in chunk order (W_1: operand columns folded back: hi + lo of the raw pair share a weight);
// workgroup 0 also adds the loss partials in workgroup order: *loss = sum / (3 n)
__global__ void __launch_bounds__(256) reduce_kernel(const float* __restrict__ slab, int chunks, const Plan p, float* __restrict__ grads,
                                                    const float* __restrict__ loss_part, int n_parts, float inv_count, float* __restrict__ loss) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < p.n_params) {
    int s0 = q, s1 = -1;
    if (q < p.H * p.C) {
      const int o = q / p.C, c = q % p.C;
      s0 = p.n_params + o * kCodeLd + (c < 2 ? c : c + 2);
      if (c < 2) s1 = s0 + 2;
    }
    grads[q] = ordered_sum(slab, chunks, p.slab_stride, s0, s1);
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    float s = 0.0f;
    for (int b = threadIdx.x; b < n_parts; b += 64) s += loss_part[b];
    s = wave_sum(s);
    if (threadIdx.x == 0) *loss = s * inv_count;
  }
}

struct Layout {
  int64_t n_pad;
  size_t code, h, dz, dpre, loss_part, slab, total;
};
static Layout layout(const Plan& p, int64_t n) {
  Layout s{};
  s.n_pad = (n + kTile - 1) / kTile * kTile;
  const size_t np = (size_t)s.n_pad;
  size_t o = 0;
  int64_t chunk, chunks;
  chunking(n, &chunk, &chunks);
  s.code = take(&o, np * kCodeLd * 2);
  s.h = take(&o, np * p.H * 2 * p.layers);
  s.dz = take(&o, np * p.H * 2 * p.layers);
  s.dpre = take(&o, np * kDpreLd * 2);
  s.loss_part = take(&o, kLossParts * 4);
  s.slab = take(&o, (size_t)chunks * p.slab_stride * 4);
  s.total = o;
  return s;
}
// H = 256: one layer fills the LDS of a CU
static int grid_for(const Plan& p, int64_t tiles) { return nerf::grid_for(tiles, p.H == 256 ? 1 : 2, kLossParts); }
static int lds_bytes(const Plan& p) { return p.mt * (p.ks > kCodeKs ? p.ks : kCodeKs) * 1024; }

typedef void (*ChainKernel)(Args);
static ChainKernel fwd_kernel_of(int H, bool train) {
  switch (H) {
    case 64: return train ? fwd_kernel<64, true> : fwd_kernel<64, false>;
    case 128: return train ? fwd_kernel<128, true> : fwd_kernel<128, false>;
    default: return train ? fwd_kernel<256, true> : fwd_kernel<256, false>;
  }
}
static ChainKernel dgrad_kernel_of(int H) { return H == 64 ? dgrad_kernel<64> : (H == 128 ? dgrad_kernel<128> : dgrad_kernel<256>); }

}  // namespace p1
}  // namespace nerf

using namespace nerf;

#define P1_PLAN(what)                                                                                                   \
  p1::Plan plan;                                                                                                        \
  if (!p1::make_plan(L_embed, use_pe, hidden, layers, &plan))                                                           \
    return fail(NERF_ENOSYS, what ": L_embed=%d use_pe=%d hidden=%d layers=%d (compiled: hidden 64/128/256, 1..8 layers, L_embed 0..15)", \
                L_embed, use_pe, hidden, layers)

extern "C" int64_t nerf_p1_param_count(int L_embed, int use_pe, int hidden, int layers) {
  p1::Plan plan;
  if (!p1::make_plan(L_embed, use_pe, hidden, layers, &plan)) {
    fail(NERF_ENOSYS, "nerf_p1_param_count: L_embed=%d use_pe=%d hidden=%d layers=%d is not compiled", L_embed, use_pe, hidden, layers);
    return -1;
  }
  return plan.n_params;
}
extern "C" size_t nerf_p1_packed_bytes(int L_embed, int use_pe, int hidden, int layers) {
  p1::Plan plan;
  return p1::make_plan(L_embed, use_pe, hidden, layers, &plan) ? p1::packed_bytes(plan) : 0;
}
extern "C" size_t nerf_p1_workspace_bytes(int64_t n, int L_embed, int use_pe, int hidden, int layers) {
  p1::Plan plan;
  return n > 0 && p1::make_plan(L_embed, use_pe, hidden, layers, &plan) ? p1::layout(plan, n).total : 0;
}

extern "C" int nerf_p1_pack(const float* params_f32, int L_embed, int use_pe, int hidden, int layers, void* packed, nerf_stream_t stream) {
  P1_PLAN("nerf_p1_pack");
  NERF_REQUIRE(params_f32 && packed && ((uintptr_t)packed & 255) == 0, "nerf_p1_pack: bad pointer");
  int blocks = (plan.frags * 64 + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(p1::pack_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), params_f32, static_cast<char*>(packed), plan);
  return check_launch("nerf_p1_pack");
}

extern "C" int nerf_p1_fwd(const void* packed, const float* coords, int64_t n, int L_embed, int use_pe, int hidden, int layers, float* y,
                           nerf_stream_t stream) {
  P1_PLAN("nerf_p1_fwd");
  NERF_REQUIRE(n >= 0, "nerf_p1_fwd: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && coords && y, "nerf_p1_fwd: NULL pointer");
  p1::Args a{};
  a.packed = static_cast<const char*>(packed); a.p = plan; a.coords = coords; a.y = y;
  a.n = n; a.n_pad = (n + p1::kTile - 1) / p1::kTile * p1::kTile;
  const int waves = p1::fwd_waves(hidden, false);
  const int grid = p1::grid_for(plan, a.n_pad / (32 * waves));
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p1_fwd: cannot query device");
  return p1::launch_chain(p1::fwd_kernel_of(hidden, false), grid, 64 * waves, p1::lds_bytes(plan), stream, "nerf_p1_fwd", a);
}

extern "C" int nerf_p1_fwd_loss_bwd(const void* packed, void* workspace, const float* coords, const int64_t* idx, const float* target,
                                    int64_t n, int L_embed, int use_pe, int hidden, int layers, float* grads_f32, float* loss_accum,
                                    nerf_stream_t stream) {
  P1_PLAN("nerf_p1_fwd_loss_bwd");
  NERF_REQUIRE(n > 0, "nerf_p1_fwd_loss_bwd: n=%lld", (long long)n);
  NERF_REQUIRE(packed && workspace && coords && target && grads_f32 && loss_accum && ((uintptr_t)workspace & 255) == 0,
               "nerf_p1_fwd_loss_bwd: bad pointer");
  const p1::Layout l = p1::layout(plan, n);
  char* w = static_cast<char*>(workspace);
  p1::Args a{};
  a.packed = static_cast<const char*>(packed); a.p = plan; a.coords = coords; a.idx = idx; a.target = target;
  a.n = n; a.n_pad = l.n_pad; a.dscale = (float)(2.0 / (3.0 * (double)n));
  a.loss_part = reinterpret_cast<float*>(w + l.loss_part);
  a.code = reinterpret_cast<__bf16*>(w + l.code); a.h = reinterpret_cast<__bf16*>(w + l.h);
  a.dz = reinterpret_cast<__bf16*>(w + l.dz); a.dpre = reinterpret_cast<__bf16*>(w + l.dpre);
  const int grid = p1::grid_for(plan, a.n_pad / p1::kTile);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p1_fwd_loss_bwd: cannot query device");
  const int lds = p1::lds_bytes(plan);
  int rc = p1::launch_chain(p1::fwd_kernel_of(hidden, true), grid, p1::kThreads, lds, stream, "nerf_p1_fwd_loss_bwd (forward)", a);
  if (rc != NERF_OK) return rc;
  rc = p1::launch_chain(p1::dgrad_kernel_of(hidden), grid, p1::kThreads, lds, stream, "nerf_p1_fwd_loss_bwd (dgrad)", a);
  if (rc != NERF_OK) return rc;
  int64_t chunk, chunks;
  p1::chunking(n, &chunk, &chunks);
  p1::WgradArgs g{};
  g.p = plan; g.code = a.code; g.h = a.h; g.dz = a.dz; g.dpre = a.dpre; g.n = n; g.n_pad = l.n_pad; g.chunk = chunk;
  g.slab = reinterpret_cast<float*>(w + l.slab);
  const int jobs = layers * (hidden / p1::kOBlock) + 1;
  hipLaunchKernelGGL(p1::wgrad_kernel, dim3((unsigned)chunks, (unsigned)jobs), dim3(256), 0, as_stream(stream), g);
  if (rc = check_launch("nerf_p1_fwd_loss_bwd (wgrad)"); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(p1::reduce_kernel, dim3((plan.n_params + 255) / 256), dim3(256), 0, as_stream(stream), g.slab, (int)chunks, plan,
                     grads_f32, a.loss_part, grid, (float)(1.0 / (3.0 * (double)n)), loss_accum);
  return check_launch("nerf_p1_fwd_loss_bwd (reduce)");
}
