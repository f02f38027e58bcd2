// Instant-NGP decoder: two bias-free tiny MLPs on bf16 MFMA.
// Replaces tinycudann's FullyFusedMLP networks behind InstantNeRFDecoder (reference
// src/decoders.py:90-162):
//   sigma-net  32 -> 64 (relu) -> 16 (linear);  sigma = softplus(h[0] - 5)
//   colour-net [h (16) | dir code (27)] -> 64 (relu) -> 64 (relu) -> 3 (sigmoid)
// PARITY UNPINNED against tinycudann itself (source and binary absent); the checker is the build's
// own CPU restatement (oracle/nerf_oracle.py::instant_decoder).
//
// The resident-weight register chain of resident_chain.h: 32 samples per wave on the MFMA
// column, activations carried as accumulator tiles -> bf16 B fragments.  All 26 (forward) /
// 20 (transposed) weight fragments stay resident in LDS for the whole launch.  The kernel
// bodies are instant_chain_body.h's (shared with p4mlp.hip's canonical chain) under IPolicy; its
// density-only body (S1, S2: 8 fragments) is the chain of nerf_instant_grid_update.
// Parameter vector (fp32, [out,in] row-major, bias-free):
//   sigma_net : W1 [64,32] | W2 [16,64]                       = 3072
//   color_net : W1 [64,48] (cols 43..47 unused) | W2 [64,64] | W3 [16,64] (rows 3..15 unused) = 8192
#include "instant_chain_body.h"
#include "mlp_wgrad.h"

namespace nerf {
using namespace resident;

constexpr int kSW1 = 0, kSW2 = 2048, kCW1 = 3072, kCW2 = 6144, kCW3 = 10240, kIParams = 11264;
constexpr int kIFwdFrags = 26, kIBwdFrags = 20;
constexpr size_t kIPackBytes = (size_t)(kIFwdFrags + kIBwdFrags) * 1024;
constexpr int kIThreads = 256, kITile = 128;
static_assert(kIThreads == kInstantThreads && kITile == kInstantTile, "both kernels run instant_chain_body.h's geometry");

// fragment index of (step, m-tile, k-step); forward steps 0..4 = S1 S2 C1 C2 C3, backward 5..9 = C3t C2t C1t S2t S1t
constexpr Step istep(int s) {
  switch (s) {
    case 0: return {2, 0, 2, 0};     // S1: hash(32, nat) -> 64
    case 1: return {1, 4, 0, 4};     // S2: 64 -> 16
    case 2: return {2, 1, 2, 8};     // C1: [h16 | denc(32 nat)] -> 64
    case 3: return {2, 4, 0, 14};    // C2: 64 -> 64
    case 4: return {1, 4, 0, 22};    // C3: 64 -> 3
    case 5: return {2, 0, 1, 26};    // C3^T: d(rgb_pre) (nat) -> d(hc2)
    case 6: return {2, 4, 0, 28};    // C2^T
    case 7: return {1, 4, 0, 36};    // C1^T (h16 rows only)
    case 8: return {2, 1, 0, 40};    // S2^T: d(h16) -> d(hs1)
    default: return {1, 4, 0, 42};   // S1^T: d(hs1) -> d(hash features)
  }
}

__device__ __forceinline__ int isrc(int step, int row, int k, bool nat) {
  switch (step) {
    case 0: return kSW1 + row * 32 + k;
    case 1: return row < 16 ? kSW2 + row * 64 + k : -1;
    case 2: return nat ? (k < 27 ? kCW1 + row * 48 + 16 + k : -1) : (k < 16 ? kCW1 + row * 48 + k : -1);
    case 3: return kCW2 + row * 64 + k;
    case 4: return row < 3 ? kCW3 + row * 64 + k : -1;
    case 5: return k < 3 ? kCW3 + k * 64 + row : -1;
    case 6: return kCW2 + k * 64 + row;
    case 7: return row < 16 ? kCW1 + k * 48 + row : -1;
    case 8: return k < 16 ? kSW2 + k * 64 + row : -1;
    default: return row < 32 ? kSW1 + k * 32 + row : -1;
  }
}

__global__ void __launch_bounds__(256) ipack_kernel(const float* __restrict__ params, __bf16* __restrict__ packed) {
  pack_fragments(params, reinterpret_cast<char*>(packed), kIFwdFrags + kIBwdFrags, 10, istep, isrc, [](int) { return false; },
                 blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

struct IArgs {
  const char* packed;
  const __bf16* hash_nat;   // nat blocks [n_pad,32] from nerf_hash_encode_fwd
  const float* dirs;        // [n,3] unit view directions
  const float* x_enc;       // encoded entry (InstantNeRFDecoder.forward(x_enc, d_enc)): [n,32] hash features and
  const float* d_enc;       // [n,27] direction codes given by the caller; NULL: hash_nat image + dirs
  __bf16* hash_nat_out;     // encoded entry, training: the feature image the wgrad pass reads is written here
  int64_t n, n_pad;
  float* rgb;               // [n,3]
  float* sigma;             // [n]
  // training stash (blocked images) and relu bits
  __bf16* hs1; __bf16* h16; __bf16* denc; __bf16* hc1; __bf16* hc2;
  uint4* mask;              // [tiles][256]
  // backward
  const float* d_rgb; const float* d_sigma;
  __bf16* dzs1; __bf16* dzs2; __bf16* dzc1; __bf16* dzc2; __bf16* dsmall;
  float* d_feat;            // [n,32] fp32
  float2* grad_lm;          // instead of d_feat: level-major gradients [16][n] float2 (the binned hash backward's input)
  unsigned* amax_bits;      // kAmaxSlots words: running maxima of |d_feat| as fp32 bits (the scatter's fixed-point scale)
  float* zero_grads;        // backward: the weight-gradient vector [kIParams], cleared here for the wgrad launch that follows and ADDS
};

// what instant_chain_body.h needs to know of this decoder: bf16 operands, two natural k-steps of hash features into the sigma-net;
// one m-tile at a time in the forward (kFence): unfenced, the shared body measured 1 % behind the file's former own body, fenced it
// needs 188 VGPRs instead of 300 and is 10 ... 16 % ahead of it
struct IPolicy {
  static constexpr StepFn step_of = istep;
  enum { S1, S2, C1, C2, C3, C3t, C2t, C1t, S2t, S1t };
  static constexpr int kFwd0 = 0, kFwdN = kIFwdFrags, kBwd0 = kIFwdFrags, kBwdN = kIBwdFrags;   // istep().frag0 counts from the forward stream
  static constexpr int kSigmaKs = 2, kParams = kIParams;
  static constexpr bool kZeroGrads = true, kFence = true;
  using V = bf16x8;
  using Mfma = MfmaBf;
  // the sigma-net's input alone (instant_sigma): the two natural k-steps of the hash operand image
  template <class A>
  static __device__ __forceinline__ void sigma_operands(const A& a, int64_t wt, int col, int half, bf16x8 (&hin)[2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) hin[ks] = load_nat<bf16x8>(a.hash_nat, wt, 2, ks, col, half);
  }
  template <bool TRAIN>
  static __device__ __forceinline__ void operands(const IArgs& a, int64_t wt, int64_t nc, int col, int half, bf16x8 (&hin)[2], bf16x8 (&denc)[2]) {
    if (a.x_enc != nullptr) {
      // already-encoded inputs (src/decoders.py:136-162 as a stand-alone operator)
      encoded_operand<2, 32>(a.x_enc + nc * 32, half, hin);
      encoded_operand<2, plan::kDirDim>(a.d_enc + nc * plan::kDirDim, half, denc);
      if constexpr (TRAIN) {
        stash_nat(a.hash_nat_out, wt, 2, 0, col, half, hin[0]);
        stash_nat(a.hash_nat_out, wt, 2, 1, col, half, hin[1]);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) hin[ks] = load_nat<bf16x8>(a.hash_nat, wt, 2, ks, col, half);
      fourier_operand<2, plan::kDirDim>(a.dirs[nc * 3 + 0], a.dirs[nc * 3 + 1], a.dirs[nc * 3 + 2], half, denc);
    }
    if constexpr (TRAIN) {
      stash_nat(a.denc, wt, 2, 0, col, half, denc[0]);
      stash_nat(a.denc, wt, 2, 1, col, half, denc[1]);
    }
  }
};

template <bool TRAIN>
__global__ void __launch_bounds__(kIThreads) imlp_fwd_kernel(const IArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  instant_forward<IPolicy, TRAIN>(a, smem, tid, lane, wave, col, half);
}

// The inference chain with the sample count read from DEVICE memory (nerf_instant_render_rays_fwd): the launch is sized for `capacity`
// samples, the unchanged body runs on n = *count (clamped to the capacity) -- its tile loop strides, so surplus workgroups leave it
// at once.  A count of 0 returns before a.n - 1 is formed; the test is uniform, so no barrier is left behind.
__global__ void __launch_bounds__(kIThreads) imlp_fwd_counted_kernel(const IArgs a0, const unsigned* __restrict__ count, int64_t capacity) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int64_t n = (int64_t)*count;
  if (n == 0) return;
  n = n < capacity ? n : capacity;
  IArgs a = a0;
  a.n = n;
  a.n_pad = (n + kITile - 1) / kITile * kITile;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  instant_forward<IPolicy, false>(a, smem, tid, lane, wave, col, half);
}

// The occupancy-grid refresh's chain (nerf_instant_grid_update): sigma-net only on a slab's operand image, folded into the grid
struct ISigmaArgs {
  const char* packed;
  const __bf16* hash_nat;   // nat blocks [n_pad,32] of the slab's cells
  int64_t n, n_pad;
  float* grid;              // [n] in/out, the slab's cells
  uint8_t* binary;          // [n]
  float decay; int dynamic; float threshold;
  unsigned long long* count;
};
constexpr int kISigmaFrags = istep(2).frag0;     // S1 and S2: the first 8 of the 26 forward fragments

__global__ void __launch_bounds__(kIThreads) imlp_sigma_grid_kernel(const ISigmaArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  instant_sigma<IPolicy>(a, smem, tid, lane, wave, col, half);
}

__global__ void __launch_bounds__(kIThreads) imlp_bwd_kernel(const IArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
  instant_dgrad<IPolicy>(a, smem, tid, lane, wave, col, half);
}

struct ILayout {
  int64_t n_pad;
  size_t hash_nat, hs1, h16, denc, hc1, hc2, mask, dzs1, dzs2, dzc1, dzc2, dsmall, slab, total;
};
static ILayout ilayout(int64_t n) {
  ILayout s{};
  s.n_pad = (n + kITile - 1) / kITile * kITile;
  const size_t np = (size_t)s.n_pad;
  size_t o = 0;                                 // every piece is a multiple of 256 bytes (n_pad is one of 128): take() pads nothing
  s.hash_nat = take(&o, np * 32 * 2);
  s.hs1 = take(&o, np * 64 * 2);
  s.h16 = take(&o, np * 32 * 2);
  s.denc = take(&o, np * 32 * 2);
  s.hc1 = take(&o, np * 64 * 2);
  s.hc2 = take(&o, np * 64 * 2);
  s.mask = take(&o, (np / kITile) * kIThreads * 16);
  s.dzs1 = take(&o, np * 64 * 2);
  s.dzs2 = take(&o, np * 32 * 2);
  s.dzc1 = take(&o, np * 64 * 2);
  s.dzc2 = take(&o, np * 64 * 2);
  s.dsmall = take(&o, np * 16 * 2);
  s.slab = take(&o, kSmallSlabBytes);           // partial tiles of the weight-gradient launch (option "deterministic")
  s.total = o;
  return s;
}

static IArgs iargs(const void* packed, void* ws, const float* dirs, int64_t n, float* rgb, float* sigma) {
  const ILayout l = ilayout(n);
  char* w = static_cast<char*>(ws);
  IArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.hash_nat = reinterpret_cast<const __bf16*>(w + l.hash_nat);
  a.dirs = dirs; a.n = n; a.n_pad = l.n_pad; a.rgb = rgb; a.sigma = sigma;
  a.hs1 = reinterpret_cast<__bf16*>(w + l.hs1); a.h16 = reinterpret_cast<__bf16*>(w + l.h16);
  a.denc = reinterpret_cast<__bf16*>(w + l.denc); a.hc1 = reinterpret_cast<__bf16*>(w + l.hc1);
  a.hc2 = reinterpret_cast<__bf16*>(w + l.hc2); a.mask = reinterpret_cast<uint4*>(w + l.mask);
  a.dzs1 = reinterpret_cast<__bf16*>(w + l.dzs1); a.dzs2 = reinterpret_cast<__bf16*>(w + l.dzs2);
  a.dzc1 = reinterpret_cast<__bf16*>(w + l.dzc1); a.dzc2 = reinterpret_cast<__bf16*>(w + l.dzc2);
  a.dsmall = reinterpret_cast<__bf16*>(w + l.dsmall);
  return a;
}

}  // namespace nerf

using namespace nerf;

extern "C" size_t nerf_imlp_packed_bytes(void) { return kIPackBytes; }
extern "C" size_t nerf_imlp_workspace_bytes(int64_t n) { return n > 0 ? ilayout(n).total : 0; }
extern "C" size_t nerf_imlp_hash_operand_offset(int64_t n) { return n > 0 ? ilayout(n).hash_nat : 0; }

extern "C" int nerf_imlp_pack(const float* params_f32, void* packed, nerf_stream_t stream) {
  NERF_REQUIRE(params_f32 && packed && ((uintptr_t)packed & 255) == 0, "nerf_imlp_pack: bad pointer");
  hipLaunchKernelGGL(ipack_kernel, dim3(16), dim3(256), 0, as_stream(stream), params_f32, static_cast<__bf16*>(packed));
  return check_launch("nerf_imlp_pack");
}

extern "C" int nerf_imlp_fwd(const void* packed, void* workspace, const float* dirs, int64_t n, float* rgb,
                             float* sigma, int train, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0, "nerf_imlp_fwd: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && workspace && dirs && rgb && sigma && ((uintptr_t)workspace & 255) == 0, "nerf_imlp_fwd: bad pointer");
  const IArgs a = iargs(packed, workspace, dirs, n, rgb, sigma);
  const int grid = grid_for(a.n_pad / kITile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_imlp_fwd: cannot query device");
  if (train) hipLaunchKernelGGL(imlp_fwd_kernel<true>, dim3(grid), dim3(kIThreads), kIFwdFrags * 1024, as_stream(stream), a);
  else hipLaunchKernelGGL(imlp_fwd_kernel<false>, dim3(grid), dim3(kIThreads), kIFwdFrags * 1024, as_stream(stream), a);
  return check_launch("nerf_imlp_fwd");
}

// inference on a device-side count (common.h; render_instant.hip's chain): only the operand image of the workspace layout exists
int nerf::imlp_fwd_counted(const void* packed, const void* hash_nat, const float* dirs, const unsigned* count, int64_t capacity, float* rgb,
                           float* sigma, nerf_stream_t stream) {
  NERF_REQUIRE(capacity > 0 && packed && hash_nat && dirs && count && rgb && sigma, "imlp_fwd_counted: bad arguments");
  IArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.hash_nat = static_cast<const __bf16*>(hash_nat);
  a.dirs = dirs; a.rgb = rgb; a.sigma = sigma;
  const int grid = grid_for((capacity + kITile - 1) / kITile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_instant_render_rays_fwd: cannot query device");
  hipLaunchKernelGGL(imlp_fwd_counted_kernel, dim3(grid), dim3(kIThreads), kIFwdFrags * 1024, as_stream(stream), a, count, capacity);
  return check_launch("nerf_instant_render_rays_fwd (decoder)");
}

// the density-only chain of one slab of grid cells (common.h; grid.hip's nerf_instant_grid_update has checked its arguments)
int nerf::imlp_sigma_grid(const void* packed, const void* hash_nat, int64_t n_cells, float* grid, uint8_t* binary_grid, float decay, int dynamic,
                          float threshold, unsigned long long* active_count, nerf_stream_t stream) {
  NERF_REQUIRE(n_cells > 0 && packed && hash_nat && grid && binary_grid && active_count, "imlp_sigma_grid: bad arguments");
  ISigmaArgs a{};
  a.packed = static_cast<const char*>(packed);
  a.hash_nat = static_cast<const __bf16*>(hash_nat);
  a.n = n_cells; a.n_pad = (n_cells + kITile - 1) / kITile * kITile;
  a.grid = grid; a.binary = binary_grid; a.decay = decay; a.dynamic = dynamic; a.threshold = threshold; a.count = active_count;
  // two workgroups per CU: every workgroup ends with one atomic on the count word, and those retire one after the other (~11 ns each) --
  // measured on a 2^18-cell slab: 1 per CU 13.5 us, 2: 12.8, 4: 17.3, 8: 28.7
  const int wgs = grid_for(a.n_pad / kITile, 2);
  if (wgs <= 0) return fail(NERF_ELAUNCH, "nerf_instant_grid_update: cannot query device");
  hipLaunchKernelGGL(imlp_sigma_grid_kernel, dim3(wgs), dim3(kIThreads), kISigmaFrags * 1024, as_stream(stream), a);
  return check_launch("nerf_instant_grid_update (sigma-net)");
}

extern "C" int nerf_imlp_fwd_encoded(const void* packed, void* workspace, const float* x_enc, const float* d_enc, int64_t n,
                                     float* rgb, float* sigma, int train, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0, "nerf_imlp_fwd_encoded: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(packed && workspace && x_enc && d_enc && rgb && sigma && ((uintptr_t)workspace & 255) == 0, "nerf_imlp_fwd_encoded: bad pointer");
  IArgs a = iargs(packed, workspace, nullptr, n, rgb, sigma);
  a.x_enc = x_enc; a.d_enc = d_enc;
  a.hash_nat_out = const_cast<__bf16*>(a.hash_nat);
  const int grid = grid_for(a.n_pad / kITile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_imlp_fwd_encoded: cannot query device");
  if (train) hipLaunchKernelGGL(imlp_fwd_kernel<true>, dim3(grid), dim3(kIThreads), kIFwdFrags * 1024, as_stream(stream), a);
  else hipLaunchKernelGGL(imlp_fwd_kernel<false>, dim3(grid), dim3(kIThreads), kIFwdFrags * 1024, as_stream(stream), a);
  return check_launch("nerf_imlp_fwd_encoded");
}

static int imlp_bwd_impl(const void* packed, void* workspace, const float* rgb, const float* sigma, const float* d_rgb,
                         const float* d_sigma, int64_t n, float* grads_f32, float* d_feat, float2* grad_lm, unsigned* amax_bits,
                         nerf_stream_t stream);

extern "C" int nerf_imlp_bwd(const void* packed, void* workspace, const float* rgb, const float* sigma,
                             const float* d_rgb, const float* d_sigma, int64_t n, float* grads_f32,
                             float* d_feat, nerf_stream_t stream) {
  NERF_REQUIRE(n == 0 || d_feat != nullptr, "nerf_imlp_bwd: d_feat is NULL");
  return imlp_bwd_impl(packed, workspace, rgb, sigma, d_rgb, d_sigma, n, grads_f32, d_feat, nullptr, nullptr, stream);
}

// row-major feature gradients AND their largest magnitude (amax_bits: device u32, max-accumulated fp32 bits; the caller zeroes it):
// what the speculative hash backward needs without the level-major copy (whose stores cost this kernel 33 us on 200 k points)
extern "C" int nerf_imlp_bwd_amax(const void* packed, void* workspace, const float* rgb, const float* sigma,
                                  const float* d_rgb, const float* d_sigma, int64_t n, float* grads_f32,
                                  float* d_feat, void* amax_bits, nerf_stream_t stream) {
  NERF_REQUIRE(n == 0 || (d_feat != nullptr && amax_bits != nullptr), "nerf_imlp_bwd_amax: NULL output");
  return imlp_bwd_impl(packed, workspace, rgb, sigma, d_rgb, d_sigma, n, grads_f32, d_feat, nullptr, static_cast<unsigned*>(amax_bits), stream);
}

extern "C" int nerf_imlp_bwd_lm(const void* packed, void* workspace, const float* rgb, const float* sigma,
                                const float* d_rgb, const float* d_sigma, int64_t n, float* grads_f32,
                                void* grad_lm, void* amax_bits, nerf_stream_t stream) {
  NERF_REQUIRE(n == 0 || (grad_lm != nullptr && amax_bits != nullptr), "nerf_imlp_bwd_lm: NULL output");
  return imlp_bwd_impl(packed, workspace, rgb, sigma, d_rgb, d_sigma, n, grads_f32, nullptr, static_cast<float2*>(grad_lm),
                       static_cast<unsigned*>(amax_bits), stream);
}

static int imlp_bwd_impl(const void* packed, void* workspace, const float* rgb, const float* sigma, const float* d_rgb,
                         const float* d_sigma, int64_t n, float* grads_f32, float* d_feat, float2* grad_lm, unsigned* amax_bits,
                         nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && grads_f32, "nerf_imlp_bwd: bad arguments");
  if (n == 0) {
    if (hipMemsetAsync(grads_f32, 0, sizeof(float) * kIParams, as_stream(stream)) != hipSuccess)
      return fail(NERF_ELAUNCH, "nerf_imlp_bwd: memset failed");
    return NERF_OK;
  }
  NERF_REQUIRE(packed && workspace && rgb && sigma && d_rgb && d_sigma && (d_feat || grad_lm), "nerf_imlp_bwd: NULL pointer");
  IArgs a = iargs(packed, workspace, nullptr, n, const_cast<float*>(rgb), const_cast<float*>(sigma));
  a.d_rgb = d_rgb; a.d_sigma = d_sigma; a.d_feat = d_feat; a.grad_lm = grad_lm; a.amax_bits = amax_bits;
  a.zero_grads = grads_f32;            // the dgrad kernel clears the vector the wgrad launch behind it adds to
  const int grid = grid_for(a.n_pad / kITile, 4);
  if (grid <= 0) return fail(NERF_ELAUNCH, "nerf_imlp_bwd: cannot query device");
  hipLaunchKernelGGL(imlp_bwd_kernel, dim3(grid), dim3(kIThreads), kIBwdFrags * 1024, as_stream(stream), a);
  int rc = check_launch("nerf_imlp_bwd (dgrad)");
  if (rc != NERF_OK) return rc;
  // weight gradients: five small jobs on the shared split-K kernel
  const ILayout l = ilayout(n);
  const char* w = static_cast<const char*>(workspace);
  WgradArgs wa{};
  { WgradJob j = make_job(w, l.dzs1, 4096, 2, 0, 0, l.hash_nat, 1, 6); j.w_off = kSW1; j.w_ld = 32; j.o_valid = 64; j.nat_valid = 32; wa.jobs[0] = j; }
  instant_common_jobs(wa, w, InstantImages{l.hs1, l.h16, l.denc, l.hc1, l.hc2, l.dzs2, l.dzc1, l.dzc2, l.dsmall}, kSW2, kCW1, kCW2, kCW3);
  wa.n_jobs = 5;
  if (options().deterministic)      // partial tiles summed in workgroup order instead of one float atomic per weight and workgroup
    return wgrad_launch(wa, n, grads_f32, as_stream(stream), reinterpret_cast<float*>(static_cast<char*>(workspace) + l.slab), kSmallSlabBytes);
  return wgrad_launch(wa, n, grads_f32, as_stream(stream));
}
