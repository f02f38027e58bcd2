// What the sample-major fused chains (p1fit.hip, p2chain.hip) share: the register chain's staging and tile loop, the
// sample-axis weight-gradient job, the ordered chunk sum and the host-side chunking / launch helpers.
//
// The chain: 32 samples per wave on the MFMA column (v_mfma_f32_32x32x16_bf16), accumulator tiles -> bf16 B fragments of the next
// step, ONE step's weight fragments at a time staged from the packed fragment image (L2) into LDS.  Each engine keeps its plan, its
// pack source map, its code operand, its chain kernels, its job table and its C entries; every __global__ entry point stays in its
// own file and namespace.
#pragma once
#include "mlp_chain.h"

namespace nerf {
namespace sample_chain {

// ------------------------------------------------------------------------------------------------ staging and tiles
// one step's fragments: packed image -> LDS by direct-to-LDS loads (no data registers): one wave instruction moves one 1-KiB
// fragment, lane l its bytes [16 l, 16 l + 16).  The first barrier: every wave is done with the previous step.  Then every wave
// waits for its OWN loads (vmcnt 0; the other counters at their maxima) before the second barrier, which makes all of them visible.
constexpr int kWaitVm0 = (15 << 8) | (7 << 4);       // s_waitcnt immediate: vmcnt(0), expcnt and lgkmcnt not waited for
template <int WAVES>
__device__ __forceinline__ void stage(char* smem, const char* src, int frags) {
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = wave; i < frags; i += WAVES)
    __builtin_amdgcn_global_load_lds((gptr_t)(src + (size_t)i * 1024 + lane * 16), (lptr_t)(smem + i * 1024), 16, 0, 0);
  __builtin_amdgcn_s_waitcnt(kWaitVm0);
  __syncthreads();
}

// output tiles M0..M1-1 of one step (tile M0's fragments first at wbase): acc = bias (or 0) + A B, then epi(m, acc).  AHEAD: the
// read-ahead depth of the m-tile (H = 256 holds two 64-register operand arrays and reads 2 fragments ahead: 3 spilled registers)
template <int M0, int M1, int KS, int AHEAD, class Epi>
__device__ __forceinline__ void run(const char* wbase, const bf16x8 (&b)[KS], const float* bias, int half, Epi&& epi) {
  static_for<M1 - M0>([&](auto ic) {
    constexpr int i = decltype(ic)::value, m = M0 + i;
    f32x16 acc;
    if (bias != nullptr) acc = bias_tile(bias, 32 * m, half);
    else {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    }
    acc = mtile<KS, AHEAD>(wbase, i * KS, b, acc);
    epi(std::integral_constant<int, m>{}, acc);
    __builtin_amdgcn_sched_barrier(0);       // one tile at a time: interleaved tiles cost registers (H = 256 spilled)
  });
}

// the two operand fragments of an accumulator tile hold features 32 m + 8 g + 4 half + (0..3), g = 0..3: four runs of 4
__device__ __forceinline__ void store_rows(__bf16* img, int ld, int64_t n, int m, int half, const bf16x8& lo, const bf16x8& hi) {
  __bf16* row = img + n * ld + 32 * m + 4 * half;
  *reinterpret_cast<bf16x4*>(row + 0) = bf16x4{lo[0], lo[1], lo[2], lo[3]};
  *reinterpret_cast<bf16x4*>(row + 8) = bf16x4{lo[4], lo[5], lo[6], lo[7]};
  *reinterpret_cast<bf16x4*>(row + 16) = bf16x4{hi[0], hi[1], hi[2], hi[3]};
  *reinterpret_cast<bf16x4*>(row + 24) = bf16x4{hi[4], hi[5], hi[6], hi[7]};
}
__device__ __forceinline__ void load_rows(const __bf16* img, int ld, int64_t n, int m, int half, float (&out)[16]) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(img + n * ld + 32 * m + 8 * g + 4 * half);
#pragma unroll
    for (int r = 0; r < 4; ++r) out[4 * g + r] = (float)v[r];
  }
}

// ------------------------------------------------------------------------------------------------ weight-gradient job
// weight gradients: chunk-partial tiles of every parameter, then one ordered sum
constexpr int kMaxChunks = 64, kMinChunk = 1024, kSub = 32, kOBlock = 64;
constexpr int kALd = kOBlock + 4, kBLd = 256 + 4;

// Weight gradients of one block of 64 output features over one chunk of samples: dW[o][i] = sum_n A[n][o] B[n][i],
// db[o] = sum_n A[n][o], with the SAMPLES on the MFMA k axis.
struct Job {
  const __bf16* A; const __bf16* B;
  int a_ld, O, o0;           // A: row stride, valid output features, first feature of this block
  int b_ld, I;               // B: row stride = columns staged (a multiple of 8, at most 256), valid input columns
  int w_off, w_ld, b_off;    // dW[o][i] -> slab[w_off + o * w_ld + i]; db -> slab[b_off + o] (b_off < 0: none)
};
// Samples n0..n1-1 of one job, by one workgroup of 256 threads.  32 samples at a time are staged row-major in LDS (padded rows:
// the two lane halves read rows 8 apart from disjoint banks) and read back transposed, element by element, into fragments.
// Wave w owns input tiles w and w + 4 of both output tiles.  The chunk's tiles are STORED into its slab row `out`.
__device__ __forceinline__ void wgrad_job(const Job& jb, int64_t n0, int64_t n1, float* out) {
  __shared__ __attribute__((aligned(16))) __bf16 As[kSub * kALd];
  __shared__ __attribute__((aligned(16))) __bf16 Bs[kSub * kBLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  const __bf16 *A = jb.A, *B = jb.B;
  const int a_ld = jb.a_ld, O = jb.O, o0 = jb.o0, b_ld = jb.b_ld, I = jb.I;
  const int n_ot = o0 + 32 < O ? 2 : 1;
  f32x16 acc[2][2];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q >> 1][q & 1][r] = 0.0f;
  float bsum = 0.0f;
  for (int64_t s0 = n0; s0 < n1; s0 += kSub) {
    __syncthreads();
    {
      const int s = tid >> 3, c = 8 * (tid & 7);
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (s0 + s < n1 && o0 + c < a_ld) v = *reinterpret_cast<const uint4*>(A + (s0 + s) * a_ld + o0 + c);
      uint2* dst = reinterpret_cast<uint2*>(As + s * kALd + c);
      dst[0] = make_uint2(v.x, v.y); dst[1] = make_uint2(v.z, v.w);
    }
    const int groups = b_ld >> 3;
    for (int e = tid; e < kSub * groups; e += 256) {
      const int s = e / groups, c = 8 * (e % groups);
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (s0 + s < n1) v = *reinterpret_cast<const uint4*>(B + (s0 + s) * b_ld + c);
      uint2* dst = reinterpret_cast<uint2*>(Bs + s * kBLd + c);
      dst[0] = make_uint2(v.x, v.y); dst[1] = make_uint2(v.z, v.w);
    }
    __syncthreads();
    if (tid < kOBlock) {
      for (int s = 0; s < kSub; ++s) bsum += (float)As[s * kALd + tid];
    }
#pragma unroll
    for (int kk = 0; kk < kSub / 16; ++kk) {
      const int srow = 16 * kk + 8 * half;
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int j = 0; j < 8; ++j) fa[t][j] = As[(srow + j) * kALd + 32 * t + col];
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int it = wave + 4 * t;
        if (32 * it < b_ld) {
#pragma unroll
          for (int j = 0; j < 8; ++j) fb[t][j] = Bs[(srow + j) * kBLd + 32 * it + col];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) fb[t][j] = (__bf16)0.0f;
        }
      }
#pragma unroll
      for (int ot = 0; ot < 2; ++ot) {
        if (ot < n_ot) {
#pragma unroll
          for (int t = 0; t < 2; ++t)
            if (32 * (wave + 4 * t) < b_ld) acc[ot][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[ot], fb[t], acc[ot][t], 0, 0, 0);
        }
      }
    }
  }
  // accumulator register r of lane (col, half): output feature 8 (r >> 2) + 4 half + (r & 3), input column col
#pragma unroll
  for (int ot = 0; ot < 2; ++ot) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int i = 32 * (wave + 4 * t) + col;
      if (ot >= n_ot || i >= I) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int o = o0 + 32 * ot + 8 * (r >> 2) + 4 * half + (r & 3);
        if (o < O) out[jb.w_off + o * jb.w_ld + i] = acc[ot][t][r];
      }
    }
  }
  if (jb.b_off >= 0 && tid < kOBlock && o0 + tid < O) out[jb.b_off + o0 + tid] = bsum;
}

// ------------------------------------------------------------------------------------------------ reduction
// sum over the chunks' slab rows of column q (q2 >= 0: of column q plus column q2), in chunk order
__device__ __forceinline__ float ordered_sum(const float* __restrict__ slab, int chunks, int stride, int q, int q2 = -1) {
  float s = 0.0f;
  for (int c = 0; c < chunks; ++c) {
    const float* row = slab + (size_t)c * stride;
    s += q2 >= 0 ? row[q] + row[q2] : row[q];
  }
  return s;
}

// ------------------------------------------------------------------------------------------------ host helpers
static void chunking(int64_t n, int64_t* chunk, int64_t* chunks) {
  // chunks of at least kMinChunk samples (multiples of kSub), at most kMaxChunks of them
  int64_t c = (n + kMinChunk - 1) / kMinChunk;
  if (c > kMaxChunks) c = kMaxChunks;
  int64_t len = (n + c - 1) / c;
  len = (len + kSub - 1) / kSub * kSub;
  *chunk = len;
  *chunks = (n + len - 1) / len;
}
template <class A>
static int launch_chain(void (*kernel)(A), int grid, int threads, int lds, nerf_stream_t stream, const char* what, const A& args) {
  if (int rc = ensure_dynamic_lds((const void*)kernel, lds, what); rc != NERF_OK) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, as_stream(stream), args);
  return check_launch(what);
}

}  // namespace sample_chain
}  // namespace nerf
