// Vanilla NeRF decoder at non-default shapes (reference src/decoders.py:29-87 behind NeuralField('part2_nerf'), src/core.py:36-55,
// with the Fourier codes of src/embeddings.py:22-32) as a sample-major fused chain, with its backward and weight gradients:
//
//   x = o + d z, v = d / |d|              ray mode (reference src/renderer.py:288-299); point mode: x, v as given
//   h_0  = relu(W_0 code(x) + b_0)                          C -> H            C = 3 + 6 L_embed
//   h_l  = relu(W_l h_{l-1} + b_l)          l = 1..layers-1 H -> H            (l = skip_layer: W_l [h_{l-1} | code(x)])
//   sigma = relu(w_s h_last + b_s)                          H -> 1
//   f    = W_f h_last + b_f                                 H -> H            (linear)
//   h_v  = relu(W_v [f | code(v)] + b_v)                    H + D -> V        D = 3 + 6 L_embed_dir
//   rgb  = sigmoid(W_c h_v + b_c)                           V -> 3
//
// Compiled: H in {64, 128, 256}, 2..8 layers (a runtime loop for a templated H), skip_layer 1..layers-1 or none,
// V in {64, 128}, L_embed 1..10 (one 64-column operand), L_embed_dir 0..4 (one 32-column operand).  The view layer always runs at
// 128 rows: V = 64 pads W_v / b_v / W_c with zeros (relu(0) = 0, masks false: the pad rows carry nothing in either direction).
//
// The sample-major register chain of sample_chain.h (staging, tile loop, image rows, the weight-gradient job and the host helpers
// live there): 32 samples per wave on the MFMA column (v_mfma_f32_32x32x16_bf16), accumulator tiles -> bf16 B fragments of the
// next layer, ONE layer's weights at a time staged from the packed fragment image into LDS (the skip layer in
// two halves of its output tiles: 8 x (16 + 4) fragments would fill all 160 KiB).  bf16 operands, fp32 accumulation, fp32 biases
// as the accumulators' initial values: the rounding points of the vanilla chain (mlp_fwd.hip) and of p3canon.hip.  The codes are
// formed in registers with the arithmetic of fourier.hip ((x * 2^band) * pi, both products rounded, full-range sine / cosine) and
// formed AGAIN at the skip layer instead of being held live (the same bits).
//
// Training images are row-major bf16: code [n_pad][64], code(v) [n_pad][32], h_0..h_last [n_pad][H], f [n_pad][H], h_v
// [n_pad][128]; the relu masks are h > 0 of the stored values.  The dgrad kernel runs the transposed chain from d rgb, d sigma
// (through sigmoid', the bare relu of sigma, the view layer, the linear feature layer, the trunk with the skip layer's hidden
// columns only: positions and directions are not learned) and writes the pre-activation gradient images.  Weight and bias
// gradients: chunk-partial tiles over the sample axis on bf16 MFMA (sample_chain.h::wgrad_job with this decoder's job table), then
// one reduction in chunk order.  No float atomics anywhere: the same bits on every run.
//
// tools/kernel_resources.py p2:: lists the registers (scratch 0 and no spills in every kernel).
//
// Parameter vector (fp32, the module's state dict concatenated, [out, in] row-major):
//   pts_layers.l.{weight,bias} l = 0..layers-1 | sigma_layer | feature_layer | view_layer | rgb_layer
#include <math.h>
#include "sample_chain.h"

namespace nerf {
namespace p2 {
using namespace sample_chain;

constexpr int kCodeLd = 64, kCodeKs = kCodeLd / 16, kDirLd = 32, kDirKs = kDirLd / 16, kSmallLd = 8;
constexpr int kVPad = 128, kVT = kVPad / 32, kVKs = kVPad / 16;
constexpr int kMaxLayers = 8, kMaxL = 10, kMaxLd = 4;
constexpr int kPadRows = 256;      // images are padded to a multiple of every kernel's workgroup tile

enum Kind { F0, HID, HEAD, VIEW, RGB, RGB_T, VIEW_T, HEAD_T, HID_T };
constexpr int kMaxSegs = 2 * kMaxLayers + 6;

// fragment plan (1-KiB fragments) and parameter offsets of one shape
struct Plan {
  int H, layers, skip, V, L, Ld, C, D, mt, ks;
  int n_segs, seg_start[kMaxSegs + 1];
  unsigned char seg_kind[kMaxSegs], seg_layer[kMaxSegs];
  int f0, hid[kMaxLayers], head, view, rgb, rgb_t, view_t, head_t, hid_t[kMaxLayers], frags, lds_frags;
  int w_off[kMaxLayers], b_off[kMaxLayers], w_sig, b_sig, w_feat, b_feat, w_view, b_view, w_rgb, b_rgb, n_params, slab_stride;
  __host__ __device__ int in_dim(int l) const { return l == 0 ? C : (l == skip ? H + C : H); }
  // k-steps per output tile of a step, and how many of them are in accumulator order (the rest: natural order)
  __host__ __device__ int kpt(int kind, int l) const {
    switch (kind) {
      case F0: return kCodeKs;
      case HID: return l == skip ? ks + kCodeKs : ks;
      case VIEW: return ks + kDirKs;
      case RGB: case VIEW_T: return kVKs;
      case RGB_T: return 1;
      case HEAD_T: return ks + 1;
      default: return ks;
    }
  }
  __host__ __device__ int k_acc(int kind) const {
    switch (kind) {
      case F0: case RGB_T: return 0;
      case RGB: case VIEW_T: return kVKs;
      default: return ks;
    }
  }
  __host__ __device__ int tiles(int kind) const {
    switch (kind) {
      case HEAD: return mt + 1;
      case VIEW: case RGB_T: return kVT;
      case RGB: return 1;
      default: return mt;
    }
  }
  // bias table (fp32, after the fragments): trunk [layers][H] | feature [H] | sigma (32) | view (128) | rgb (32)
  __host__ __device__ int bias_feat() const { return layers * H; }
  __host__ __device__ int bias_sig() const { return layers * H + H; }
  __host__ __device__ int bias_view() const { return bias_sig() + 32; }
  __host__ __device__ int bias_rgb() const { return bias_view() + kVPad; }
  __host__ __device__ int bias_floats() const { return bias_rgb() + 32; }
  __host__ __device__ size_t bias_bytes_off() const { return (size_t)frags * 1024; }
};

// NULL, or the key this build is not compiled for
static const char* make_plan(int H, int layers, int skip, int V, int L, int Ld, Plan* p) {
  if (!(H == 64 || H == 128 || H == 256)) return "hidden_dim";
  if (layers < 2 || layers > kMaxLayers) return "num_layers";
  if (skip == 0) return "skip_layer";
  if (!(V == 64 || V == 128)) return "view_dim";
  if (L < 1 || L > kMaxL) return "L_embed";
  if (Ld < 0 || Ld > kMaxLd) return "L_embed_dir";
  *p = Plan{};
  p->H = H; p->layers = layers; p->skip = (skip >= 1 && skip < layers) ? skip : -1; p->V = V; p->L = L; p->Ld = Ld;
  p->C = 3 + 6 * L; p->D = 3 + 6 * Ld; p->mt = H / 32; p->ks = H / 16;
  int f = 0, s = 0, lds = 0;
  auto seg = [&](int kind, int l) {
    const int count = p->tiles(kind) * p->kpt(kind, l);
    p->seg_start[s] = f; p->seg_kind[s] = (unsigned char)kind; p->seg_layer[s] = (unsigned char)l; ++s;
    const int staged = (kind == HID && l == p->skip) ? count / 2 : count;
    if (staged > lds) lds = staged;
    const int at = f;
    f += count;
    return at;
  };
  p->f0 = seg(F0, 0);
  for (int l = 1; l < layers; ++l) p->hid[l] = seg(HID, l);
  p->head = seg(HEAD, 0); p->view = seg(VIEW, 0); p->rgb = seg(RGB, 0);
  p->rgb_t = seg(RGB_T, 0); p->view_t = seg(VIEW_T, 0); p->head_t = seg(HEAD_T, 0);
  for (int l = 1; l < layers; ++l) p->hid_t[l] = seg(HID_T, l);
  p->n_segs = s; p->seg_start[s] = f; p->frags = f; p->lds_frags = lds;
  int o = 0;
  for (int l = 0; l < layers; ++l) { p->w_off[l] = o; o += H * p->in_dim(l); p->b_off[l] = o; o += H; }
  p->w_sig = o; o += H; p->b_sig = o; o += 1;
  p->w_feat = o; o += H * H; p->b_feat = o; o += H;
  p->w_view = o; o += V * (H + p->D); p->b_view = o; o += V;
  p->w_rgb = o; o += 3 * V; p->b_rgb = o; o += 3;
  p->n_params = o; p->slab_stride = (o + 63) / 64 * 64;
  return nullptr;
}
static size_t packed_bytes(const Plan& p) { return (p.bias_bytes_off() + (size_t)p.bias_floats() * 4 + 255) / 256 * 256; }

// flat parameter index feeding A[row][k] of a step, or -1 for a structural zero; nat: k counts the natural-order columns
__device__ __forceinline__ int src_index(const Plan& p, int kind, int l, int row, int k, bool nat) {
  const int H = p.H, V = p.V;
  switch (kind) {
    case F0: return k < p.C ? p.w_off[0] + row * p.C + k : -1;
    case HID: return nat ? (k < p.C ? p.w_off[l] + row * (H + p.C) + H + k : -1) : p.w_off[l] + row * p.in_dim(l) + k;
    case HEAD: return row < H ? p.w_feat + row * H + k : (row == H ? p.w_sig + k : -1);
    case VIEW:
      if (row >= V) return -1;
      return nat ? (k < p.D ? p.w_view + row * (H + p.D) + H + k : -1) : p.w_view + row * (H + p.D) + k;
    case RGB: return row < 3 && k < V ? p.w_rgb + row * V + k : -1;
    case RGB_T: return row < V && k < 3 ? p.w_rgb + k * V + row : -1;
    case VIEW_T: return k < V ? p.w_view + k * (H + p.D) + row : -1;
    case HEAD_T: return nat ? (k == 0 ? p.w_sig + row : -1) : p.w_feat + k * H + row;
    default: return p.w_off[l] + k * p.in_dim(l) + row;       // HID_T: the hidden columns of pts_layers.l, transposed
  }
}

__global__ void __launch_bounds__(256) pack_kernel(const float* __restrict__ params, char* __restrict__ packed, const Plan p) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < p.frags * 64; t += gridDim.x * blockDim.x) {
    const int frag = t >> 6, lane = t & 63, h = lane >> 5;
    int s = 0;
    while (s + 1 < p.n_segs && frag >= p.seg_start[s + 1]) ++s;
    const int kind = p.seg_kind[s], l = p.seg_layer[s], rel = frag - p.seg_start[s];
    const int kpt = p.kpt(kind, l), k_acc = p.k_acc(kind), mt = rel / kpt, ks = rel % kpt;
    const bool nat = ks >= k_acc;
    const int row = mt * 32 + (lane & 31);
    unsigned short out[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = frag_column(nat ? ks - k_acc : ks, h, j, nat);
      const int src = src_index(p, kind, l, row, k, nat);
      out[j] = __builtin_bit_cast(unsigned short, (__bf16)(src >= 0 ? params[src] : 0.0f));
    }
    store_fragment(packed, frag, lane, out);
  }
  float* bias = reinterpret_cast<float*>(packed + p.bias_bytes_off());
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < p.bias_floats(); i += gridDim.x * blockDim.x) {
    float b = 0.0f;
    if (i < p.bias_feat()) b = params[p.b_off[i / p.H] + i % p.H];
    else if (i < p.bias_sig()) b = params[p.b_feat + i - p.bias_feat()];
    else if (i < p.bias_view()) b = i == p.bias_sig() ? params[p.b_sig] : 0.0f;
    else if (i < p.bias_rgb()) b = i - p.bias_view() < p.V ? params[p.b_view + i - p.bias_view()] : 0.0f;
    else b = i - p.bias_rgb() < 3 ? params[p.b_rgb + i - p.bias_rgb()] : 0.0f;
    bias[i] = b;
  }
}

struct Args {
  const char* packed;
  Plan p;
  const float* o;            // ray mode: rays_o [R,3]; point mode: pts [n,3]
  const float* d;            // ray mode: rays_d [R,3]; point mode: dirs [n,3] (encoded as given)
  const float* z;            // [n] = [R, n_samples] (ray mode)
  int n_samples;             // 0: point mode
  int64_t n, n_pad;
  float* rgb;                // [n,3]
  float* sigma;              // [n]
  const float* d_rgb; const float* d_sigma;                       // backward
  __bf16* code; __bf16* dcode; __bf16* h; __bf16* feat; __bf16* hv;          // forward images; h: [layers][n_pad][H]
  __bf16* drgb; __bf16* dsig; __bf16* dzv; __bf16* dfeat; __bf16* dz;        // gradient images; dz: [layers][n_pad][H]
};

// KSN k-steps of the code of one triple, natural order: column f = 16 ks + 8 half + j of
// [x(3) | sin(2^0 pi x)(3) | cos(2^0 pi x)(3) | sin(2^1 pi x)(3) | ...] (src/embeddings.py:28-32), zero from column 3 + 6 L on.
// One rolled loop over the lane's 8 KSN columns (one inlined sine / cosine, not 8 KSN of them: their large-argument reduction is
// long); the bf16 results are merged into the fragment words by selects, so no register array is indexed at run time.
template <int KSN>
__device__ __forceinline__ void code_operand(float x0, float x1, float x2, int L, int half, bf16x8 (&out)[KSN]) {
  unsigned w[4 * KSN];
#pragma unroll
  for (int q = 0; q < 4 * KSN; ++q) w[q] = 0u;
  const int width = 3 + 6 * L;
#pragma unroll 1
  for (int e = 0; e < 8 * KSN; ++e) {
    const int ks = e >> 3, j = e & 7;
    if (16 * ks >= width) break;       // wave-uniform: bands past L cost no sine
    const int f = 16 * ks + 8 * half + j, c = f - 3, band = c / 6, rem = c - 6 * band, axis = f < 3 ? f : (rem >= 3 ? rem - 3 : rem);
    const float xa = axis == 0 ? x0 : (axis == 1 ? x1 : x2);
    float v = 0.0f;
    if (f < 3) v = xa;
    else if (band < L) {
      // (x * 2^band) * pi, both products rounded to fp32 (src/embeddings.py:30-31)
      const float arg = mul_rn(mul_rn(xa, (float)(1u << band)), 3.14159265358979323846f);
      float sn, cs;
      sincosf(arg, &sn, &cs);
      v = rem >= 3 ? cs : sn;
    }
    const unsigned bits = (unsigned)__builtin_bit_cast(unsigned short, (__bf16)v) << (16 * (j & 1));
#pragma unroll
    for (int q = 0; q < 4 * KSN; ++q) w[q] |= q == (e >> 1) ? bits : 0u;
  }
#pragma unroll
  for (int ks = 0; ks < KSN; ++ks) out[ks] = __builtin_bit_cast(bf16x8, u32x4{w[4 * ks], w[4 * ks + 1], w[4 * ks + 2], w[4 * ks + 3]});
}

// position and view direction of sample nc (clamped to a live row)
__device__ __forceinline__ void sample_inputs(const Args& a, int64_t nc, float (&x)[3], float (&v)[3]) {
  if (a.n_samples > 0) {
    const int64_t ray = nc / a.n_samples;
    const float zz = a.z[nc];
    float dd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      dd[c] = a.d[ray * 3 + c];
      x[c] = add_rn(a.o[ray * 3 + c], mul_rn(dd[c], zz));
    }
    const float nrm = sqrtf(add_rn(add_rn(mul_rn(dd[0], dd[0]), mul_rn(dd[1], dd[1])), mul_rn(dd[2], dd[2])));
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = dd[c] / nrm;
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) { x[c] = a.o[nc * 3 + c]; v[c] = a.d[nc * 3 + c]; }
  }
}

// H = 256 runs 4 waves per workgroup in the chain kernels: two 64-register operand arrays, the skip layer's code (forward) or the
// extra sigma k-step (dgrad) and the sample do not fit 256 registers
constexpr int fwd_waves(int H) { return H == 256 ? 4 : 8; }
constexpr int ahead(int H) { return H == 256 ? 2 : kAhead; }

template <int H, bool TRAIN>
__global__ void __launch_bounds__((64 * fwd_waves(H))) fwd_kernel(const Args a) {
  constexpr int MT = H / 32, KS = H / 16, WAVES = fwd_waves(H), AH = ahead(H);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = smem + lane * 16;
  const float* bias = reinterpret_cast<const float*>(a.packed + a.p.bias_bytes_off());
  const int layers = a.p.layers, skip = a.p.skip, L = a.p.L, Ld = a.p.Ld;
  const int64_t n_tiles = a.n_pad / (WAVES * 32);
  const size_t img = (size_t)a.n_pad * H;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t n = (tile * WAVES + wave) * 32 + col;
    const bool live = n < a.n;
    float x[3], v[3];
    sample_inputs(a, live ? n : a.n - 1, x, v);
    auto relu_epi = [&](bf16x8* out, __bf16* himg, int ld) {
      return [=](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
        acc_to_operand_relu<true>(acc, out[2 * m], out[2 * m + 1]);
        if constexpr (TRAIN) store_rows(himg, ld, n, m, half, out[2 * m], out[2 * m + 1]);
      };
    };
    bf16x8 hc[KS];
    {
      bf16x8 code[kCodeKs];
      code_operand<kCodeKs>(x[0], x[1], x[2], L, half, code);
      if constexpr (TRAIN) {
#pragma unroll
        for (int ks = 0; ks < kCodeKs; ++ks) *reinterpret_cast<bf16x8*>(a.code + n * kCodeLd + 16 * ks + 8 * half) = code[ks];
      }
      stage<WAVES>(smem, a.packed + (size_t)a.p.f0 * 1024, MT * kCodeKs);
      run<0, MT, kCodeKs, AH>(wbase, code, bias, half, relu_epi(hc, a.h, H));
    }
#pragma unroll 1
    for (int l = 1; l < layers; ++l) {
      bf16x8 hn[KS];
      const char* src = a.packed + (size_t)a.p.hid[l] * 1024;
      if (l == skip) {
        // [h_{l-1} | code(x)], hidden first (src/decoders.py:73); the code is formed again: the same arithmetic on the same values
        bf16x8 cat[KS + kCodeKs], again[kCodeKs];
        code_operand<kCodeKs>(x[0], x[1], x[2], L, half, again);
#pragma unroll
        for (int k = 0; k < KS; ++k) cat[k] = hc[k];
#pragma unroll
        for (int ks = 0; ks < kCodeKs; ++ks) cat[KS + ks] = again[ks];
        constexpr int HALF_FRAGS = (MT / 2) * (KS + kCodeKs);
        stage<WAVES>(smem, src, HALF_FRAGS);
        run<0, MT / 2, KS + kCodeKs, AH>(wbase, cat, bias + l * H, half, relu_epi(hn, a.h + l * img, H));
        stage<WAVES>(smem, src + (size_t)HALF_FRAGS * 1024, HALF_FRAGS);
        run<MT / 2, MT, KS + kCodeKs, AH>(wbase, cat, bias + l * H, half, relu_epi(hn, a.h + l * img, H));
      } else {
        stage<WAVES>(smem, src, MT * KS);
        run<0, MT, KS, AH>(wbase, hc, bias + l * H, half, relu_epi(hn, a.h + l * img, H));
      }
#pragma unroll
      for (int k = 0; k < KS; ++k) hc[k] = hn[k];
    }
    // feature_layer (linear) and sigma_layer (bare relu) on h_last (src/decoders.py:77-80)
    bf16x8 cat[KS + kDirKs];
    stage<WAVES>(smem, a.packed + (size_t)a.p.head * 1024, (MT + 1) * KS);
    run<0, MT, KS, AH>(wbase, hc, bias + a.p.bias_feat(), half, [&](auto mc, f32x16 acc) {
      constexpr int m = decltype(mc)::value;
      acc_to_operand(acc, cat[2 * m], cat[2 * m + 1]);
      if constexpr (TRAIN) store_rows(a.feat, H, n, m, half, cat[2 * m], cat[2 * m + 1]);
    });
    run<0, 1, KS, AH>(wbase + MT * KS * 1024, hc, nullptr, half, [&](auto, f32x16 acc) {
      if (live && half == 0) a.sigma[n] = fmaxf(acc[0] + bias[a.p.bias_sig()], 0.0f);
    });
    // view_layer on [f | code(v)] (relu), rgb_layer (sigmoid) (src/decoders.py:83-85)
    {
      bf16x8 dc[kDirKs];
      code_operand<kDirKs>(v[0], v[1], v[2], Ld, half, dc);
#pragma unroll
      for (int ks = 0; ks < kDirKs; ++ks) {
        cat[KS + ks] = dc[ks];
        if constexpr (TRAIN) *reinterpret_cast<bf16x8*>(a.dcode + n * kDirLd + 16 * ks + 8 * half) = dc[ks];
      }
    }
    bf16x8 hv[kVKs];
    stage<WAVES>(smem, a.packed + (size_t)a.p.view * 1024, kVT * (KS + kDirKs));
    run<0, kVT, KS + kDirKs, AH>(wbase, cat, bias + a.p.bias_view(), half, relu_epi(hv, a.hv, kVPad));
    stage<WAVES>(smem, a.packed + (size_t)a.p.rgb * 1024, kVKs);
    run<0, 1, kVKs, AH>(wbase, hv, nullptr, half, [&](auto, f32x16 acc) {
      if (live && half == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.rgb[n * 3 + c] = 1.0f / (1.0f + expf(-(acc[c] + bias[a.p.bias_rgb() + c])));
      }
    });
  }
}

template <int H>
__global__ void __launch_bounds__((64 * fwd_waves(H))) dgrad_kernel(const Args a) {
  constexpr int MT = H / 32, KS = H / 16, AH = ahead(H), kBwdWaves = fwd_waves(H);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = smem + lane * 16;
  const int layers = a.p.layers;
  const int64_t n_tiles = a.n_pad / (kBwdWaves * 32);
  const size_t img = (size_t)a.n_pad * H;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t n = (tile * kBwdWaves + wave) * 32 + col;
    // output-layer derivatives: sigmoid' and the bare relu of sigma (zero rows beyond n)
    bf16x8 srgb[1], ssig;
#pragma unroll
    for (int j = 0; j < 8; ++j) { srgb[0][j] = (__bf16)0.0f; ssig[j] = (__bf16)0.0f; }
    if (n < a.n && half == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float r = a.rgb[n * 3 + c];
        srgb[0][c] = (__bf16)(a.d_rgb[n * 3 + c] * r * (1.0f - r));
      }
      ssig[0] = (__bf16)(a.sigma[n] > 0.0f ? a.d_sigma[n] : 0.0f);
    }
    if (half == 0) {
      *reinterpret_cast<bf16x8*>(a.drgb + n * kSmallLd) = srgb[0];
      *reinterpret_cast<bf16x8*>(a.dsig + n * kSmallLd) = ssig;
    }
    // d h -> dz = d h [h > 0] (stored activations): bf16 operand of the next transposed step + image for the weight gradients
    auto grad_epi = [&](bf16x8* out, const __bf16* h, __bf16* dz, int ld) {
      return [=](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
        if (h != nullptr) {
          float hv[16];
          load_rows(h, ld, n, m, half, hv);
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = hv[r] > 0.0f ? acc[r] : 0.0f;
        }
        acc_to_operand(acc, out[2 * m], out[2 * m + 1]);
        store_rows(dz, ld, n, m, half, out[2 * m], out[2 * m + 1]);
      };
    };
    bf16x8 gv[kVKs];
    stage<kBwdWaves>(smem, a.packed + (size_t)a.p.rgb_t * 1024, kVT);
    run<0, kVT, 1, AH>(wbase, srgb, nullptr, half, grad_epi(gv, a.hv, a.dzv, kVPad));
    bf16x8 in[KS + 1];
    stage<kBwdWaves>(smem, a.packed + (size_t)a.p.view_t * 1024, MT * kVKs);
    run<0, MT, kVKs, AH>(wbase, gv, nullptr, half, grad_epi(in, nullptr, a.dfeat, H));       // the feature layer is linear
    in[KS] = ssig;
    bf16x8 g[KS];
    stage<kBwdWaves>(smem, a.packed + (size_t)a.p.head_t * 1024, MT * (KS + 1));
    run<0, MT, KS + 1, AH>(wbase, in, nullptr, half, grad_epi(g, a.h + (layers - 1) * img, a.dz + (layers - 1) * img, H));
#pragma unroll 1
    for (int l = layers - 1; l >= 1; --l) {
      stage<kBwdWaves>(smem, a.packed + (size_t)a.p.hid_t[l] * 1024, MT * KS);
      bf16x8 gn[KS];
      run<0, MT, KS, AH>(wbase, g, nullptr, half, grad_epi(gn, a.h + (l - 1) * img, a.dz + (l - 1) * img, H));
#pragma unroll
      for (int k = 0; k < KS; ++k) g[k] = gn[k];
    }
  }
}

// Weight gradients (sample_chain.h::wgrad_job); a chunk's slab row has the layout of the parameter vector.  blockIdx.x: chunk,
// blockIdx.y: job.
struct WgradArgs {
  Plan p;
  const __bf16* code; const __bf16* dcode; const __bf16* h; const __bf16* feat; const __bf16* hv;
  const __bf16* drgb; const __bf16* dsig; const __bf16* dzv; const __bf16* dfeat; const __bf16* dz;
  int64_t n, n_pad, chunk;
  float* slab;               // [chunks][slab_stride]
};
// jobs: trunk layers x blocks | skip layer's code columns x blocks | feature x blocks | sigma | view (f columns) x 2 |
// view (direction columns) x 2 | rgb
__host__ __device__ inline int job_count(const Plan& p) {
  const int blocks = p.H / kOBlock;
  return p.layers * blocks + (p.skip > 0 ? blocks : 0) + blocks + 1 + 2 * (p.V / kOBlock) + 1;
}
__device__ __forceinline__ Job job_of(const WgradArgs& a, int job) {
  const Plan& p = a.p;
  const int H = p.H, blocks = H / kOBlock, vblocks = p.V / kOBlock;
  const size_t img = (size_t)a.n_pad * H;
  Job j{};
  if (job < p.layers * blocks) {
    const int l = job / blocks;
    j.A = a.dz + l * img; j.a_ld = H; j.O = H; j.o0 = (job % blocks) * kOBlock;
    if (l == 0) { j.B = a.code; j.b_ld = kCodeLd; j.I = p.C; }
    else { j.B = a.h + (l - 1) * img; j.b_ld = H; j.I = H; }
    j.w_off = p.w_off[l]; j.w_ld = p.in_dim(l); j.b_off = p.b_off[l];
    return j;
  }
  job -= p.layers * blocks;
  if (p.skip > 0) {
    if (job < blocks) {
      j.A = a.dz + p.skip * img; j.a_ld = H; j.O = H; j.o0 = job * kOBlock;
      j.B = a.code; j.b_ld = kCodeLd; j.I = p.C;
      j.w_off = p.w_off[p.skip] + H; j.w_ld = H + p.C; j.b_off = -1;
      return j;
    }
    job -= blocks;
  }
  if (job < blocks) {
    j.A = a.dfeat; j.a_ld = H; j.O = H; j.o0 = job * kOBlock;
    j.B = a.h + (p.layers - 1) * img; j.b_ld = H; j.I = H;
    j.w_off = p.w_feat; j.w_ld = H; j.b_off = p.b_feat;
    return j;
  }
  job -= blocks;
  if (job == 0) {
    j.A = a.dsig; j.a_ld = kSmallLd; j.O = 1; j.o0 = 0;
    j.B = a.h + (p.layers - 1) * img; j.b_ld = H; j.I = H;
    j.w_off = p.w_sig; j.w_ld = H; j.b_off = p.b_sig;
    return j;
  }
  job -= 1;
  if (job < 2 * vblocks) {
    const bool dir = job >= vblocks;
    j.A = a.dzv; j.a_ld = kVPad; j.O = p.V; j.o0 = (job % vblocks) * kOBlock;
    if (dir) { j.B = a.dcode; j.b_ld = kDirLd; j.I = p.D; j.w_off = p.w_view + H; j.b_off = -1; }
    else { j.B = a.feat; j.b_ld = H; j.I = H; j.w_off = p.w_view; j.b_off = p.b_view; }
    j.w_ld = H + p.D;
    return j;
  }
  j.A = a.drgb; j.a_ld = kSmallLd; j.O = 3; j.o0 = 0;
  j.B = a.hv; j.b_ld = kVPad; j.I = p.V;
  j.w_off = p.w_rgb; j.w_ld = p.V; j.b_off = p.b_rgb;
  return j;
}
__global__ void __launch_bounds__(256) wgrad_kernel(const WgradArgs a) {
  const Job jb = job_of(a, blockIdx.y);
  const int64_t n0 = blockIdx.x * a.chunk;
  const int64_t n1 = n0 + a.chunk < a.n ? n0 + a.chunk : a.n;
  wgrad_job(jb, n0, n1, a.slab + (size_t)blockIdx.x * a.p.slab_stride);
}

// grads[q] = sum over chunks, in chunk order
__global__ void __launch_bounds__(256) reduce_kernel(const float* __restrict__ slab, int chunks, int stride, int n_params,
                                                    float* __restrict__ grads) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n_params) grads[q] = ordered_sum(slab, chunks, stride, q);
}

struct Layout {
  int64_t n_pad;
  size_t code, dcode, h, feat, hv, drgb, dsig, dzv, dfeat, dz, slab, total;
};
static Layout layout(const Plan& p, int64_t n) {
  Layout s{};
  s.n_pad = (n + kPadRows - 1) / kPadRows * kPadRows;
  const size_t np = (size_t)s.n_pad;
  size_t o = 0;
  int64_t chunk, chunks;
  chunking(n, &chunk, &chunks);
  s.code = take(&o, np * kCodeLd * 2);
  s.dcode = take(&o, np * kDirLd * 2);
  s.h = take(&o, np * p.H * 2 * p.layers);
  s.feat = take(&o, np * p.H * 2);
  s.hv = take(&o, np * kVPad * 2);
  s.drgb = take(&o, np * kSmallLd * 2);
  s.dsig = take(&o, np * kSmallLd * 2);
  s.dzv = take(&o, np * kVPad * 2);
  s.dfeat = take(&o, np * p.H * 2);
  s.dz = take(&o, np * p.H * 2 * p.layers);
  s.slab = take(&o, (size_t)chunks * p.slab_stride * 4);
  s.total = o;
  return s;
}
static int lds_bytes(const Plan& p) { return p.lds_frags * 1024; }

typedef void (*ChainKernel)(Args);
static ChainKernel fwd_kernel_of(int H, bool train) {
  switch (H) {
    case 64: return train ? fwd_kernel<64, true> : fwd_kernel<64, false>;
    case 128: return train ? fwd_kernel<128, true> : fwd_kernel<128, false>;
    default: return train ? fwd_kernel<256, true> : fwd_kernel<256, false>;
  }
}
static ChainKernel dgrad_kernel_of(int H) { return H == 64 ? dgrad_kernel<64> : (H == 128 ? dgrad_kernel<128> : dgrad_kernel<256>); }
// forward and dgrad run the same geometry; H = 256: one step fills the LDS of a CU
static int launch(ChainKernel kernel, const Args& a, nerf_stream_t stream, const char* what) {
  const int waves = fwd_waves(a.p.H);
  const int grid = grid_for(a.n_pad / (32 * waves), a.p.H == 256 ? 1 : 2);
  if (grid <= 0) return fail(NERF_ELAUNCH, "%s: cannot query device", what);
  return launch_chain(kernel, grid, 64 * waves, lds_bytes(a.p), stream, what, a);
}

static int forward(const char* what, const void* packed, void* workspace, const float* rays_o, const float* rays_d, const float* z,
                   int64_t n, int n_samples, const Plan& plan, float* rgb, float* sigma, bool train, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && n < ((int64_t)1 << 31) && n_samples >= 0, "%s: n=%lld n_samples=%d", what, (long long)n, n_samples);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && rays_o && rays_d && rgb && sigma && ((uintptr_t)packed & 255) == 0, "%s: bad pointer", what);
  NERF_REQUIRE(n_samples == 0 || (z != nullptr && n % n_samples == 0), "%s: ray mode needs z and n = rays x n_samples", what);
  NERF_REQUIRE(!train || (workspace && ((uintptr_t)workspace & 255) == 0), "%s: training needs an aligned workspace", what);
  const Layout l = layout(plan, n);
  Args a{};
  a.packed = static_cast<const char*>(packed); a.p = plan; a.o = rays_o; a.d = rays_d; a.z = z; a.n_samples = n_samples;
  a.n = n; a.n_pad = l.n_pad; a.rgb = rgb; a.sigma = sigma;
  if (train) {
    char* w = static_cast<char*>(workspace);
    a.code = reinterpret_cast<__bf16*>(w + l.code); a.dcode = reinterpret_cast<__bf16*>(w + l.dcode);
    a.h = reinterpret_cast<__bf16*>(w + l.h); a.feat = reinterpret_cast<__bf16*>(w + l.feat); a.hv = reinterpret_cast<__bf16*>(w + l.hv);
  }
  return launch(fwd_kernel_of(plan.H, train), a, stream, what);
}

}  // namespace p2
}  // namespace nerf

using namespace nerf;

#define P2_SHAPE int hidden, int layers, int skip, int view, int L_embed, int L_dir
#define P2_PLAN(what)                                                                                                                  \
  p2::Plan plan;                                                                                                                       \
  if (const char* key = p2::make_plan(hidden, layers, skip, view, L_embed, L_dir, &plan))                                              \
    return fail(NERF_ENOSYS, what ": %s is not compiled (hidden_dim=%d num_layers=%d skip_layer=%d view_dim=%d L_embed=%d "            \
                "L_embed_dir=%d; compiled: hidden_dim 64/128/256, num_layers 2..8, skip_layer 1..num_layers-1 or none, view_dim "      \
                "64/128, L_embed 1..10, L_embed_dir 0..4)", key, hidden, layers, skip, view, L_embed, L_dir)

extern "C" int64_t nerf_p2_param_count(P2_SHAPE) {
  p2::Plan plan;
  if (const char* key = p2::make_plan(hidden, layers, skip, view, L_embed, L_dir, &plan)) {
    fail(NERF_ENOSYS, "nerf_p2_param_count: %s is not compiled (hidden_dim=%d num_layers=%d skip_layer=%d view_dim=%d L_embed=%d L_embed_dir=%d)",
         key, hidden, layers, skip, view, L_embed, L_dir);
    return -1;
  }
  return plan.n_params;
}
extern "C" size_t nerf_p2_packed_bytes(P2_SHAPE) {
  p2::Plan plan;
  return p2::make_plan(hidden, layers, skip, view, L_embed, L_dir, &plan) == nullptr ? p2::packed_bytes(plan) : 0;
}
extern "C" size_t nerf_p2_workspace_bytes(int64_t n, P2_SHAPE) {
  p2::Plan plan;
  return n > 0 && p2::make_plan(hidden, layers, skip, view, L_embed, L_dir, &plan) == nullptr ? p2::layout(plan, n).total : 0;
}

extern "C" int nerf_p2_pack(const float* params_f32, P2_SHAPE, void* packed, nerf_stream_t stream) {
  P2_PLAN("nerf_p2_pack");
  NERF_REQUIRE(params_f32 && packed && ((uintptr_t)packed & 255) == 0, "nerf_p2_pack: bad pointer");
  int blocks = (plan.frags * 64 + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(p2::pack_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), params_f32, static_cast<char*>(packed), plan);
  return check_launch("nerf_p2_pack");
}

extern "C" int nerf_p2_fwd(const void* packed, const float* rays_o, const float* rays_d, const float* z, int64_t n, int n_samples,
                           P2_SHAPE, float* rgb, float* sigma, nerf_stream_t stream) {
  P2_PLAN("nerf_p2_fwd");
  return p2::forward("nerf_p2_fwd", packed, nullptr, rays_o, rays_d, z, n, n_samples, plan, rgb, sigma, false, stream);
}

extern "C" int nerf_p2_fwd_train(const void* packed, void* workspace, const float* rays_o, const float* rays_d, const float* z, int64_t n,
                                 int n_samples, P2_SHAPE, float* rgb, float* sigma, nerf_stream_t stream) {
  P2_PLAN("nerf_p2_fwd_train");
  return p2::forward("nerf_p2_fwd_train", packed, workspace, rays_o, rays_d, z, n, n_samples, plan, rgb, sigma, true, stream);
}

extern "C" int nerf_p2_bwd(const void* packed, void* workspace, const float* rgb, const float* sigma, const float* d_rgb,
                           const float* d_sigma, int64_t n, P2_SHAPE, float* grads_f32, nerf_stream_t stream) {
  P2_PLAN("nerf_p2_bwd");
  NERF_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "nerf_p2_bwd: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && workspace && rgb && sigma && d_rgb && d_sigma && grads_f32 && ((uintptr_t)workspace & 255) == 0 &&
               ((uintptr_t)packed & 255) == 0, "nerf_p2_bwd: bad pointer");
  const p2::Layout l = p2::layout(plan, n);
  char* w = static_cast<char*>(workspace);
  auto img = [&](size_t off) { return reinterpret_cast<__bf16*>(w + off); };
  p2::Args a{};
  a.packed = static_cast<const char*>(packed); a.p = plan; a.n = n; a.n_pad = l.n_pad;
  a.rgb = const_cast<float*>(rgb); a.sigma = const_cast<float*>(sigma); a.d_rgb = d_rgb; a.d_sigma = d_sigma;
  a.h = img(l.h); a.hv = img(l.hv);
  a.drgb = img(l.drgb); a.dsig = img(l.dsig); a.dzv = img(l.dzv); a.dfeat = img(l.dfeat); a.dz = img(l.dz);
  int rc = p2::launch(p2::dgrad_kernel_of(hidden), a, stream, "nerf_p2_bwd (dgrad)");
  if (rc != NERF_OK) return rc;
  int64_t chunk, chunks;
  p2::chunking(n, &chunk, &chunks);
  p2::WgradArgs g{};
  g.p = plan; g.code = img(l.code); g.dcode = img(l.dcode); g.h = a.h; g.feat = img(l.feat); g.hv = a.hv;
  g.drgb = a.drgb; g.dsig = a.dsig; g.dzv = a.dzv; g.dfeat = a.dfeat; g.dz = a.dz;
  g.n = n; g.n_pad = l.n_pad; g.chunk = chunk; g.slab = reinterpret_cast<float*>(w + l.slab);
  hipLaunchKernelGGL(p2::wgrad_kernel, dim3((unsigned)chunks, (unsigned)p2::job_count(plan)), dim3(256), 0, as_stream(stream), g);
  if (rc = check_launch("nerf_p2_bwd (wgrad)"); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(p2::reduce_kernel, dim3((plan.n_params + 255) / 256), dim3(256), 0, as_stream(stream), g.slab, (int)chunks,
                     plan.slab_stride, plan.n_params, grads_f32);
  return check_launch("nerf_p2_bwd (reduce)");
}
