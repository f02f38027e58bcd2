// Part 3 deformation MLP (reference src/decoders.py:165-195, applied at src/core.py:262-270) as a fused register chain:
//
//   xcode = Fourier_10(x')   63 columns [x | sin(2^0 pi x) | cos(2^0 pi x) | ...]   (src/embeddings.py:22-32)
//   tcode = Fourier_10(t')   21 columns
//   h1 = relu(W1 [xcode | tcode] + b1)    84 -> 128
//   h2 = relu(W2 h1 + b2)                 128 -> 128
//   h3 = relu(W3 h2 + b3)                 128 -> 128
//   dx = W4 h3 + b4                       128 -> 3
//   x_c = x + dx                          x, NOT the noised x' (core.py:268-270)
//
// The resident-weight register chain of resident_chain.h (pack loop, LDS prologue, step runner): 32 samples per wave on the MFMA
// column, accumulator tiles -> 16-bit B fragments of the next layer, every weight fragment of one direction resident in LDS
// (forward 96 KiB fp16 + 1 KiB of biases, backward 68 KiB bf16: one workgroup of 8 waves per CU).  The forward contracts fp16
// operands (v_mfma_f32_32x32x16_f16) for the reason p4mlp.hip gives: dx moves x_c inside a canonical hash grid whose finest cells
// are ~4.3e-4 wide.  The backward and the training images are bf16.  b1 rides on a constant-1 column (84) of the layer-1 operand,
// b2 / b3 initialise the accumulators, b4 is added to the output.
//
// Training images are row-major [n_pad][width] bf16 (code 96, h1..h3 128; the relu masks are h > 0 of the stored values,
// which bf16 rounding cannot flip).  The backward runs the transposed chain on the stored masks (no input gradient: x', t'
// are not learned) and writes dz1..dz3; the weight gradients are then summed by chunk-partial tiles in a slab and ONE
// reduction in chunk order: no float atomics anywhere, the same bits on every run.
//
// Parameter vector (fp32, the module's state dict concatenated, [out, in] row-major):
//   W1 [128,84] b1 [128] W2 [128,128] b2 [128] W3 [128,128] b3 [128] W4 [3,128] b4 [3]   deform_net.net.{0,2,4,6}
#include "resident_chain.h"
#include "sample_chain.h"
#include "lattice.h"

namespace nerf {
namespace p3 {
using namespace resident;

constexpr int kIn = 84, kHid = 128, kCodeLd = 96, kTimeDim = 21, kPosDim = 63;
constexpr int kW1 = 0, kB1 = 10752, kW2 = 10880, kB2 = 27264, kW3 = 27392, kB3 = 43776, kW4 = 43904, kB4 = 44288, kParams = 44291;
constexpr int kThreads = 512, kWaves = kThreads / 64, kTile = kWaves * 32;

enum { F1, F2, F3, F4, B4t, B3t, B2t, kSteps };
constexpr Step step_of(int s) {
  switch (s) {
    case F1: return {4, 0, 6, 0};       // [xcode | tcode | 1] (96 nat) -> 128
    case F2: return {4, 8, 0, 24};      // 128 -> 128
    case F3: return {4, 8, 0, 56};
    case F4: return {1, 8, 0, 88};      // 128 -> 3
    case B4t: return {4, 0, 1, 96};     // d dx (16 nat) -> d h3
    case B3t: return {4, 8, 0, 100};    // dz3 -> d h2
    default: return {4, 8, 0, 132};     // B2t: dz2 -> d h1
  }
}
constexpr int kFrags = 164;
constexpr int kFwd0 = 0, kFwdN = 96, kBwd0 = 96, kBwdN = 68;
constexpr size_t kBiasOff = (size_t)kFrags * 1024;             // b2 [128] | b3 [128] | b4 [3] (fp32)
constexpr size_t kPackBytes = kBiasOff + 2048;
constexpr int kFwdLds = kFwdN * 1024 + 2048, kBwdLds = kBwdN * 1024;
// weight gradients: chunk-partial tiles of every parameter, then one ordered sum
constexpr int kMaxChunks = 256, kMinChunk = 1024, kSub = 32;

__device__ __forceinline__ int src_of(int step, int row, int k, bool) {
  switch (step) {
    case F1: return k < kIn ? kW1 + row * kIn + k : (k == kIn ? kB1 + row : -1);
    case F2: return kW2 + row * kHid + k;
    case F3: return kW3 + row * kHid + k;
    case F4: return row < 3 ? kW4 + row * kHid + k : -1;
    case B4t: return k < 3 ? kW4 + k * kHid + row : -1;
    case B3t: return kW3 + k * kHid + row;
    default: return kW2 + k * kHid + row;
  }
}

__global__ void __launch_bounds__(256) pack_kernel(const float* __restrict__ params, char* __restrict__ packed) {
  pack_fragments(params, packed, kFrags, kSteps, step_of, src_of, [](int step) { return step <= F4; },   // forward: fp16, backward: bf16
                 blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
  if (blockIdx.x == 0) {
    float* bias = reinterpret_cast<float*>(packed + kBiasOff);
    for (int i = threadIdx.x; i < 512; i += blockDim.x)
      bias[i] = i < 128 ? params[kB2 + i] : (i < 256 ? params[kB3 + i - 128] : (i < 259 ? params[kB4 + i - 256] : 0.0f));
  }
}

struct Args {
  const char* packed;
  const float* x_code;     // [n,3] x' (the Fourier code's input)
  const float* x;          // [n,3] x (x_c = x + dx)
  const float* t;          // [n] t'
  const float* d_dx;       // [n,3]
  int64_t n, n_pad;
  float* dx; float* xc;
  __bf16* code; __bf16* h[3]; __bf16* dz[3];   // training images [n_pad][96] / [n_pad][128]
};

// Column f >= kPosDim of the layer-1 operand at time t: [t | sin(2^0 pi t) | cos(2^0 pi t) | ... (21) | 1 | 0 ...]
__device__ __forceinline__ float time_column(int f, float t) {
  if (f < kIn) {
    const int c = f - kPosDim;
    if (c == 0) return t;
    return sincos_rev(t, (float)(1u << ((c - 1) >> 1)), ((c - 1) & 1) ? 0.25f : 0.0f);
  }
  return f == kIn ? 1.0f : 0.0f;
}
// One wave tile of the forward chain, shared by fwd_kernel and the scalar-time kernels (deform_scalar_time): the layer-1 operand of the point (x0, x1, x2)
// -- its 63 position columns are formed here; time_of(f) is the value of column f >= kPosDim (time_column's), asked for the two
// columns 16 ks + j and 16 ks + 8 + j of which the lane keeps its half's -- then F1..F3 with the ReLU epilogue and F4, whose
// accumulator tile goes to out(mc, acc).  n: the lane's row (the training images' row; unused otherwise).  FENCE: run_step's, one
// m-tile at a time.
template <bool TRAIN, bool FENCE, class TimeOf, class Out>
__device__ __forceinline__ void chain_tile(const char* wbase, const float* bias, float x0, float x1, float x2, TimeOf&& time_of, int64_t n,
                                           int half, __bf16* code_img, __bf16* const (&h_img)[3], Out&& out) {
  // layer-1 operand, natural order: column f = 16 ks + 8 half + j of [xcode (63) | tcode (21) | 1 | 0 ...]
  f16x8 code[6];
#pragma unroll
  for (int ks = 0; ks < 6; ++ks) {
    bf16x8 cb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f0 = 16 * ks + j, f1 = f0 + 8;       // this lane's column is f0 (half 0) or f1 (half 1)
      auto value = [&](int f) -> float {
        if (f < kPosDim) return feat_eval<kPosDim>(feat_spec<kPosDim>(f), x0, x1, x2);
        return time_of(f);
      };
      const float v = half ? value(f1) : value(f0);
      code[ks][j] = (_Float16)v;
      cb[j] = (__bf16)v;
    }
    if constexpr (TRAIN) *reinterpret_cast<bf16x8*>(code_img + n * kCodeLd + 16 * ks + 8 * half) = cb;
  }
  auto relu_epi = [&](f16x8* o, __bf16* img) {
    return [=](auto mc, f32x16 acc) {
      constexpr int m = decltype(mc)::value;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.0f);
      acc_to_operand16(acc, o[2 * m], o[2 * m + 1]);
      if constexpr (TRAIN) {
        bf16x8 lo, hi;
        acc_to_operand(acc, lo, hi);
        sample_chain::store_rows(img, kHid, n, m, half, lo, hi);
      }
    };
  };
  f16x8 h1[8], h2[8];
  run_step<step_of, F1, 6, FENCE>(wbase, code, nullptr, Mfma16{}, relu_epi(h1, h_img[0]));
  run_step<step_of, F2, 8, FENCE>(wbase, h1, bias, Mfma16{}, relu_epi(h2, h_img[1]));
  run_step<step_of, F3, 8, FENCE>(wbase, h2, bias + 128, Mfma16{}, relu_epi(h1, h_img[2]));
  run_step<step_of, F4, 8, FENCE>(wbase, h1, nullptr, Mfma16{}, out);
}

// forward fragments and the bias block -> LDS (the caller's barrier follows); returns the lane's A base
__device__ __forceinline__ const char* fwd_resident(char* smem, const char* packed, int tid, int lane) {
  const char* wbase = resident_weights<kThreads>(smem, packed, kFwd0, kFwdN, tid, lane);
  if (tid < 128) reinterpret_cast<uint4*>(smem + kFwdN * 1024)[tid] = reinterpret_cast<const uint4*>(packed + kBiasOff)[tid];
  return wbase;
}

template <bool TRAIN>
__global__ void __launch_bounds__(kThreads) fwd_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = fwd_resident(smem, a.packed, tid, lane);
  __syncthreads();
  const float* bias = reinterpret_cast<const float*>(smem + kFwdN * 1024);
  const int64_t n_tiles = a.n_pad / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t n = (tile * kWaves + wave) * 32 + col;
    const bool live = n < a.n;
    const int64_t nc = live ? n : a.n - 1;
    const float x0 = a.x_code[nc * 3 + 0], x1 = a.x_code[nc * 3 + 1], x2 = a.x_code[nc * 3 + 2], t = a.t[nc];
    chain_tile<TRAIN, false>(wbase, bias, x0, x1, x2, [&](int f) { return time_column(f, t); }, n, half, a.code, a.h,
                      [&](auto, f32x16 acc) {
      if (live && half == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float d = acc[c] + bias[256 + c];
          a.dx[n * 3 + c] = d;
          a.xc[n * 3 + c] = a.x[n * 3 + c] + d;
        }
      }
    });
  }
}

// The deformation chain of the occupancy-grid refresh (nerf_p3_grid_update): fwd_kernel<false> for the cells of a lattice slab at
// ONE time stamp t, storing x_c alone.  Why the bits stay fwd_kernel's:
//   * x is lattice_node of the cell index, the value nerf_grid_lattice stores; the code's input x' is x (evaluation adds no noise).
//   * t is uniform, so columns 63..95 of the layer-1 operand (t, its 20 sin / cos columns, the constant 1, the zero pad) are the same
//     in every MFMA column of every tile: formed ONCE per wave, before the tile loop, by time_column on the same value -- the
//     lane's part of k-step 3 and all of k-steps 4 and 5, as fp16.  F1 contracts them in its own k-step order, as fwd_kernel does
//     (they are NOT moved into an accumulator initialiser, which would change the fp32 summation order).
//   * x_c = x + (acc + b4), fwd_kernel's association.
struct LatticeArgs {
  const char* packed;
  float t;
  int64_t cell0, n, n_pad;   // first cell of the slab, its cells, rounded up to whole tiles
  int res;
  float bound, step;         // the lattice (lattice.h)
  float* xc;                 // [n,3]
};

// The body of the two scalar-time kernels below: rows [0, n_rows) (> 0; n_pad: rounded up to whole tiles) at the time t, the point of a
// row supplied by point_of(row, x) -- pad rows ask for row n_rows - 1 -- and x_c stored for the live rows alone.
template <class PointOf>
__device__ __forceinline__ void deform_scalar_time(char* smem, const char* packed, float t, int64_t n_rows, int64_t n_pad, float* xc,
                                                   int tid, int lane, int wave, int col, int half, PointOf point_of) {
  const char* wbase = fwd_resident(smem, packed, tid, lane);
  // tcode[ks - 3][j]: THIS LANE's column 16 ks + 8 half + j of k-steps 3..5, where it is a time column.  Lane-half 0 of k-step 3
  // holds columns 48..55, all position columns: its slots stay 0 and are never asked for.
  f16x8 tcode[3];
#pragma unroll
  for (int ks = 3; ks < 6; ++ks) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int f0 = 16 * ks + j, f1 = f0 + 8;
      const float v = half ? time_column(f1, t) : (f0 >= kPosDim ? time_column(f0, t) : 0.0f);
      tcode[ks - 3][j] = (_Float16)v;
    }
  }
  __syncthreads();
  const float* bias = reinterpret_cast<const float*>(smem + kFwdN * 1024);
  __bf16* const no_img[3] = {nullptr, nullptr, nullptr};
  const int64_t n_tiles = n_pad / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t n = (tile * kWaves + wave) * 32 + col;
    const bool live = n < n_rows;
    float x[3];
    point_of(live ? n : n_rows - 1, x);
    // chain_tile asks for columns 16 ks + j and 16 ks + 8 + j and keeps the one of the lane's half: both map to slot [ks - 3][j], which
    // holds that half's value (fp16 -> fp32 -> fp16 is exact)
    auto time_of = [&](int f) { return (float)tcode[f / 16 - 3][f % 8]; };
    chain_tile<false, true>(wbase, bias, x[0], x[1], x[2], time_of, n, half, nullptr, no_img,
                      [&](auto, f32x16 acc) {
      if (live && half == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) xc[n * 3 + c] = x[c] + (acc[c] + bias[256 + c]);
      }
    });
  }
}

__global__ void __launch_bounds__(kThreads) deform_lattice_kernel(const LatticeArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  deform_scalar_time(smem, a.packed, a.t, a.n, a.n_pad, a.xc, tid, lane, wave, col, half, [&](int64_t row, float (&x)[3]) {
    int i[3];
    lattice_cell(a.cell0 + row, a.res, i[0], i[1], i[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = lattice_node(i[c], a.res, a.bound, a.step);
  });
}

// The deformation chain of the Part 3 evaluation launch chain (nerf_p3_render_rays_fwd): the same body on the first *count rows of the
// compaction's pts at the time *time_dev, both read from DEVICE memory.  The launch is sized for `capacity` rows; the count is clamped
// to it (a count the compaction cannot produce must not become an access outside pts / xc), n == 0 leaves before n - 1 exists, and the
// padded row count is formed here.  The early return is uniform over the launch: no barrier is skipped by part of a workgroup.
__global__ void __launch_bounds__(kThreads) deform_counted_kernel(const char* packed, const float* __restrict__ pts,
                                                                  const unsigned* __restrict__ count, int64_t capacity,
                                                                  const float* __restrict__ time_dev, float* __restrict__ xc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int64_t n = (int64_t)*count;
  if (n == 0) return;
  n = n < capacity ? n : capacity;
  const float t = *time_dev;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  deform_scalar_time(smem, packed, t, n, (n + kTile - 1) / kTile * kTile, xc, tid, lane, wave, col, half, [&](int64_t row, float (&x)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = pts[row * 3 + c];
  });
}

// The deformation chain of the Part 3 (8x256 canonical field) evaluation launch chain (nerf_p3_nerf_render_rays_fwd): the same body on
// rows [0, n) of nerf_sample_rays's pts -- that field has no occupancy grid, every sample of the chunk is a row, so n (> 0) is known on
// the host -- at the time *time_dev, read from DEVICE memory once at entry.  The padded row count is formed here, as above.
__global__ void __launch_bounds__(kThreads) deform_rows_kernel(const char* packed, const float* __restrict__ pts, int64_t n,
                                                               const float* __restrict__ time_dev, float* __restrict__ xc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const float t = *time_dev;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  deform_scalar_time(smem, packed, t, n, (n + kTile - 1) / kTile * kTile, xc, tid, lane, wave, col, half, [&](int64_t row, float (&x)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = pts[row * 3 + c];
  });
}

__global__ void __launch_bounds__(kThreads) dgrad_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const char* wbase = resident_weights<kThreads>(smem, a.packed, kBwd0, kBwdN, tid, lane);
  __syncthreads();
  const int64_t n_tiles = a.n_pad / kTile;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t n = (tile * kWaves + wave) * 32 + col;
    const bool live = n < a.n;
    bf16x8 small[1];
#pragma unroll
    for (int j = 0; j < 8; ++j) small[0][j] = (__bf16)0.0f;
    if (live && half == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) small[0][c] = (__bf16)a.d_dx[n * 3 + c];
    }
    // d h_k -> dz_k = d h_k [h_k > 0] (stored activations), bf16 operand of the next transposed layer + image for the wgrad
    auto mask_epi = [&](bf16x8* out, const __bf16* h, __bf16* dz) {
      return [=](auto mc, f32x16 acc) {
        constexpr int m = decltype(mc)::value;
        float hv[16];
        sample_chain::load_rows(h, kHid, n, m, half, hv);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = hv[r] > 0.0f ? acc[r] : 0.0f;
        acc_to_operand(acc, out[2 * m], out[2 * m + 1]);
        sample_chain::store_rows(dz, kHid, n, m, half, out[2 * m], out[2 * m + 1]);
      };
    };
    bf16x8 g3[8], g2[8], g1[8];
    run_step<step_of, B4t, 1>(wbase, small, nullptr, MfmaBf{}, mask_epi(g3, a.h[2], a.dz[2]));
    run_step<step_of, B3t, 8>(wbase, g3, nullptr, MfmaBf{}, mask_epi(g2, a.h[1], a.dz[1]));
    run_step<step_of, B2t, 8>(wbase, g2, nullptr, MfmaBf{}, mask_epi(g1, a.h[0], a.dz[0]));
    (void)g1;
  }
}

// Weight gradients of one layer over one chunk of samples: dW[o][i] = sum_n A[n][o] B[n][i], db[o] = sum_n A[n][o].  Thread
// (ob, ib) owns an 8 x 8 block; samples are staged 32 at a time in LDS as fp32.  The chunk's tile is STORED into its slab row.
struct WgradArgs {
  const __bf16* code; const __bf16* h[3]; const __bf16* dz[3];
  const float* d_dx;
  int64_t n, chunk;
  float* slab;             // [chunks][kParams]
};
template <int A_LD, int B_LD, int O, int I, bool A_F32>
__device__ __forceinline__ void wgrad_layer(const void* A, const __bf16* B, int64_t n0, int64_t n1, int w_off, int b_off, float* out, char* smem) {
  float* As = reinterpret_cast<float*>(smem);                 // [kSub][A_LD]
  float* Bs = As + kSub * A_LD;                               // [kSub][B_LD]
  constexpr int OB = (O + 7) / 8, IB = (I + 7) / 8;
  const int tid = threadIdx.x;
  const bool owner = tid < OB * IB;
  const int ob = tid / IB, ib = tid % IB;
  float acc[8][8], bsum[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    bsum[p] = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[p][q] = 0.0f;
  }
  for (int64_t s0 = n0; s0 < n1; s0 += kSub) {
    const int cnt = (int)(n1 - s0 < kSub ? n1 - s0 : kSub);
    __syncthreads();
    for (int e = tid; e < kSub * A_LD; e += blockDim.x) {
      const int s = e / A_LD, c = e % A_LD;
      float v = 0.0f;
      if (s < cnt && c < O) v = A_F32 ? static_cast<const float*>(A)[(s0 + s) * 3 + c] : (float)static_cast<const __bf16*>(A)[(s0 + s) * A_LD + c];
      As[e] = v;
    }
    for (int e = tid; e < kSub * B_LD; e += blockDim.x) {
      const int s = e / B_LD;
      Bs[e] = s < cnt ? (float)B[(s0 + s) * B_LD + e % B_LD] : 0.0f;
    }
    __syncthreads();
    if (owner) {
      for (int s = 0; s < kSub; ++s) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(As + s * A_LD + 8 * ob), a1 = *reinterpret_cast<const f32x4*>(As + s * A_LD + 8 * ob + 4);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(Bs + s * B_LD + 8 * ib), b1 = *reinterpret_cast<const f32x4*>(Bs + s * B_LD + 8 * ib + 4);
        const float av[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
        const float bv[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          bsum[p] += av[p];
#pragma unroll
          for (int q = 0; q < 8; ++q) acc[p][q] = __builtin_fmaf(av[p], bv[q], acc[p][q]);
        }
      }
    }
  }
  if (!owner) return;
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int o = 8 * ob + p;
    if (o >= O) continue;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = 8 * ib + q;
      if (i < I) out[w_off + o * I + i] = acc[p][q];
    }
    if (ib == 0) out[b_off + o] = bsum[p];
  }
}

// blockIdx.x: chunk, blockIdx.y: layer.  A_LD >= 8 * ceil(O / 8) (the owner reads 8 rows of A).
__global__ void __launch_bounds__(256) wgrad_kernel(const WgradArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[kSub * (kHid + kHid) * 4];
  const int64_t n0 = blockIdx.x * a.chunk;
  const int64_t n1 = n0 + a.chunk < a.n ? n0 + a.chunk : a.n;
  float* out = a.slab + (size_t)blockIdx.x * kParams;
  switch (blockIdx.y) {
    case 0: wgrad_layer<kHid, kCodeLd, kHid, kIn, false>(a.dz[0], a.code, n0, n1, kW1, kB1, out, smem); break;
    case 1: wgrad_layer<kHid, kHid, kHid, kHid, false>(a.dz[1], a.h[0], n0, n1, kW2, kB2, out, smem); break;
    case 2: wgrad_layer<kHid, kHid, kHid, kHid, false>(a.dz[2], a.h[1], n0, n1, kW3, kB3, out, smem); break;
    default: wgrad_layer<8, kHid, 3, kHid, true>(a.d_dx, a.h[2], n0, n1, kW4, kB4, out, smem); break;
  }
}

// grads[p] += sum over chunks, in chunk order
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ slab, int chunks, float* __restrict__ grads) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= kParams) return;
  float s = 0.0f;
  for (int c = 0; c < chunks; ++c) s += slab[(size_t)c * kParams + p];
  grads[p] += s;
}

struct Layout {
  int64_t n_pad;
  size_t code, h[3], dz[3], slab, total;
};
static Layout layout(int64_t n) {
  Layout s{};
  s.n_pad = (n + kTile - 1) / kTile * kTile;
  const size_t np = (size_t)s.n_pad;
  size_t o = 0;
  s.code = take(&o, np * kCodeLd * 2);
  for (int k = 0; k < 3; ++k) s.h[k] = take(&o, np * kHid * 2);
  for (int k = 0; k < 3; ++k) s.dz[k] = take(&o, np * kHid * 2);
  s.slab = take(&o, (size_t)kMaxChunks * kParams * 4);
  s.total = o;
  return s;
}
static Args args_of(const void* packed, void* ws, int64_t n) {
  const Layout l = layout(n);
  char* w = static_cast<char*>(ws);
  Args a{};
  a.packed = static_cast<const char*>(packed);
  a.n = n; a.n_pad = l.n_pad;
  a.code = reinterpret_cast<__bf16*>(w + l.code);
  for (int k = 0; k < 3; ++k) { a.h[k] = reinterpret_cast<__bf16*>(w + l.h[k]); a.dz[k] = reinterpret_cast<__bf16*>(w + l.dz[k]); }
  return a;
}

}  // namespace p3
}  // namespace nerf

using namespace nerf;

extern "C" int64_t nerf_p3_deform_param_count(void) { return p3::kParams; }
extern "C" size_t nerf_p3_deform_packed_bytes(void) { return p3::kPackBytes; }
extern "C" size_t nerf_p3_deform_workspace_bytes(int64_t n) { return n > 0 ? p3::layout(n).total : 0; }

extern "C" int nerf_p3_deform_pack(const float* params_f32, void* packed, nerf_stream_t stream) {
  NERF_REQUIRE(params_f32 && packed && ((uintptr_t)packed & 255) == 0, "nerf_p3_deform_pack: bad pointer");
  hipLaunchKernelGGL(p3::pack_kernel, dim3(48), dim3(256), 0, as_stream(stream), params_f32, static_cast<char*>(packed));
  return check_launch("nerf_p3_deform_pack");
}

extern "C" int nerf_p3_deform_fwd(const void* packed, void* workspace, const float* x_code, const float* pts, const float* t_deform,
                                  int64_t n, float* delta_x, float* x_canonical, int train, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0, "nerf_p3_deform_fwd: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && pts && t_deform && delta_x && x_canonical, "nerf_p3_deform_fwd: NULL pointer");
  NERF_REQUIRE(!train || (workspace && ((uintptr_t)workspace & 255) == 0), "nerf_p3_deform_fwd: training needs an aligned workspace");
  p3::Args a{};
  if (train) a = p3::args_of(packed, workspace, n);
  a.packed = static_cast<const char*>(packed);
  a.n = n; a.n_pad = (n + p3::kTile - 1) / p3::kTile * p3::kTile;
  a.x_code = x_code ? x_code : pts; a.x = pts; a.t = t_deform; a.dx = delta_x; a.xc = x_canonical;
  const int grid = grid_for(a.n_pad / p3::kTile, 1);   // one workgroup per CU (LDS)
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p3_deform_fwd: cannot query device");
  const void* kernel = train ? (const void*)p3::fwd_kernel<true> : (const void*)p3::fwd_kernel<false>;
  if (int rc = ensure_dynamic_lds(kernel, p3::kFwdLds, "nerf_p3_deform_fwd"); rc != NERF_OK) return rc;
  if (train) hipLaunchKernelGGL(p3::fwd_kernel<true>, dim3(grid), dim3(p3::kThreads), p3::kFwdLds, as_stream(stream), a);
  else hipLaunchKernelGGL(p3::fwd_kernel<false>, dim3(grid), dim3(p3::kThreads), p3::kFwdLds, as_stream(stream), a);
  return check_launch("nerf_p3_deform_fwd");
}

extern "C" int nerf_p3_deform_bwd(const void* packed, void* workspace, const float* d_delta_x, int64_t n, float* grads_f32,
                                  nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && grads_f32, "nerf_p3_deform_bwd: bad arguments");
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && workspace && d_delta_x && ((uintptr_t)workspace & 255) == 0, "nerf_p3_deform_bwd: bad pointer");
  p3::Args a = p3::args_of(packed, workspace, n);
  a.d_dx = d_delta_x;
  const int grid = grid_for(a.n_pad / p3::kTile, 1);   // one workgroup per CU (LDS)
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p3_deform_bwd: cannot query device");
  if (int rc = ensure_dynamic_lds((const void*)p3::dgrad_kernel, p3::kBwdLds, "nerf_p3_deform_bwd"); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(p3::dgrad_kernel, dim3(grid), dim3(p3::kThreads), p3::kBwdLds, as_stream(stream), a);
  if (int rc = check_launch("nerf_p3_deform_bwd (dgrad)"); rc != NERF_OK) return rc;
  // chunks of at least kMinChunk samples (multiples of kSub), at most kMaxChunks of them
  int64_t chunks = (n + p3::kMinChunk - 1) / p3::kMinChunk;
  if (chunks > p3::kMaxChunks) chunks = p3::kMaxChunks;
  int64_t chunk = (n + chunks - 1) / chunks;
  chunk = (chunk + p3::kSub - 1) / p3::kSub * p3::kSub;
  chunks = (n + chunk - 1) / chunk;
  const p3::Layout l = p3::layout(n);
  p3::WgradArgs w{};
  w.code = a.code; w.d_dx = d_delta_x; w.n = n; w.chunk = chunk;
  for (int k = 0; k < 3; ++k) { w.h[k] = a.h[k]; w.dz[k] = a.dz[k]; }
  w.slab = reinterpret_cast<float*>(static_cast<char*>(workspace) + l.slab);
  hipLaunchKernelGGL(p3::wgrad_kernel, dim3((unsigned)chunks, 4), dim3(256), 0, as_stream(stream), w);
  if (int rc = check_launch("nerf_p3_deform_bwd (wgrad)"); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(p3::wgrad_reduce_kernel, dim3((p3::kParams + 255) / 256), dim3(256), 0, as_stream(stream), w.slab, (int)chunks, grads_f32);
  return check_launch("nerf_p3_deform_bwd (reduce)");
}

// The deformation launch of nerf_p3_grid_update per (slab, time) (common.h; grid.hip has checked the entry's arguments)
int nerf::p3_deform_lattice(const void* packed, float t, int64_t cell0, int64_t n_cells, int resolution, float grid_bound, float* x_canonical,
                            nerf_stream_t stream) {
  NERF_REQUIRE(cell0 >= 0 && n_cells > 0 && resolution >= 2 && packed && x_canonical, "nerf_p3_grid_update (deformation chain): bad arguments");
  p3::LatticeArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.t = t;
  a.cell0 = cell0; a.n = n_cells; a.n_pad = (n_cells + p3::kTile - 1) / p3::kTile * p3::kTile;
  a.res = resolution; a.bound = grid_bound; a.step = lattice_step(grid_bound, resolution);
  a.xc = x_canonical;
  const int grid = grid_for(a.n_pad / p3::kTile, 1);   // one workgroup per CU (LDS)
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p3_grid_update: cannot query device");
  if (int rc = ensure_dynamic_lds((const void*)p3::deform_lattice_kernel, p3::kFwdLds, "nerf_p3_grid_update"); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(p3::deform_lattice_kernel, dim3(grid), dim3(p3::kThreads), p3::kFwdLds, as_stream(stream), a);
  return check_launch("nerf_p3_grid_update (deformation chain)");
}

// The deformation launch of nerf_p3_render_rays_fwd per chunk (common.h; render_p3.hip has checked the entry's arguments): sized for the
// chunk's capacity, surplus workgroups fall out of the striding tile loop.
int nerf::p3_deform_counted(const void* packed, const float* pts, const unsigned* count, int64_t capacity, const float* time_dev,
                            float* x_canonical, nerf_stream_t stream) {
  NERF_REQUIRE(capacity > 0 && packed && pts && count && time_dev && x_canonical, "nerf_p3_render_rays_fwd (deformation chain): bad arguments");
  const int grid = grid_for((capacity + p3::kTile - 1) / p3::kTile, 1);   // one workgroup per CU (LDS)
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p3_render_rays_fwd: cannot query device");
  if (int rc = ensure_dynamic_lds((const void*)p3::deform_counted_kernel, p3::kFwdLds, "nerf_p3_render_rays_fwd"); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(p3::deform_counted_kernel, dim3(grid), dim3(p3::kThreads), p3::kFwdLds, as_stream(stream),
                     static_cast<const char*>(packed), pts, count, capacity, time_dev, x_canonical);
  return check_launch("nerf_p3_render_rays_fwd (deformation chain)");
}

// The deformation launch of nerf_p3_nerf_render_rays_fwd per chunk (common.h; render_p3_nerf.hip has checked the entry's arguments): rows
// [0, n) of the chunk's pts, n on the host.
int nerf::p3_deform_rows(const void* packed, const float* pts, int64_t n, const float* time_dev, float* x_canonical, nerf_stream_t stream) {
  NERF_REQUIRE(n > 0 && packed && pts && time_dev && x_canonical, "nerf_p3_nerf_render_rays_fwd (deformation chain): bad arguments");
  const int grid = grid_for((n + p3::kTile - 1) / p3::kTile, 1);   // one workgroup per CU (LDS)
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_p3_nerf_render_rays_fwd: cannot query device");
  if (int rc = ensure_dynamic_lds((const void*)p3::deform_rows_kernel, p3::kFwdLds, "nerf_p3_nerf_render_rays_fwd"); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(p3::deform_rows_kernel, dim3(grid), dim3(p3::kThreads), p3::kFwdLds, as_stream(stream),
                     static_cast<const char*>(packed), pts, n, time_dev, x_canonical);
  return check_launch("nerf_p3_nerf_render_rays_fwd (deformation chain)");
}
