// Adam / AdamW over one flat fp32 parameter vector: 28 B/param of streaming traffic, float4-vectorised -- and the
// fused regulariser + clip + AdamW passes of the flat hash-table groups.  The pieces the passes share stand first, each written once.
#include "common.h"

#include <type_traits>

namespace nerf {

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float lr, float beta1, float beta2,
                                            float eps, float wd, float inv_bc1, float inv_sqrt_bc2) {
  float pi = p;
  if (wd != 0.0f) pi *= (1.0f - lr * wd);
  const float mi = beta1 * m + (1.0f - beta1) * g;
  const float vi = beta2 * v + (1.0f - beta2) * g * g;
  m = mi;
  v = vi;
  p = pi - (lr * inv_bc1) * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
}

// Elements [4q, 4q + 4) of one array.  VEC: one 16-byte access (the chunk lies inside [0, n), the base is 16-byte aligned); otherwise
// element by element, zeros read and nothing written past n.
template <bool VEC>
__device__ __forceinline__ f4 load4(const float* __restrict__ a, int64_t q, int64_t n) {
  if (VEC) return reinterpret_cast<const f4*>(a)[q];
  f4 x;
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = 4 * q + e < n ? a[4 * q + e] : 0.0f;
  return x;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ a, int64_t q, int64_t n, f4 x) {
  if (VEC) { reinterpret_cast<f4*>(a)[q] = x; return; }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (4 * q + e < n) a[4 * q + e] = x[e];
}

// fp16 copy of the updated parameters (the hash forward gathers from it); shadow may be NULL
template <bool VEC>
__device__ __forceinline__ void store_shadow4(_Float16* __restrict__ shadow, int64_t q, int64_t n, f4 pp) {
  typedef _Float16 h4 __attribute__((ext_vector_type(4)));
  if (shadow == nullptr) return;
  if (VEC) { reinterpret_cast<h4*>(shadow)[q] = h4{(_Float16)pp[0], (_Float16)pp[1], (_Float16)pp[2], (_Float16)pp[3]}; return; }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (4 * q + e < n) shadow[4 * q + e] = (_Float16)pp[e];
}

// element e of a chunk (a vector's element does not bind to a reference)
__device__ __forceinline__ void adam_update(f4& pp, int e, float g, f4& mm, f4& vv, float lr, float beta1, float beta2, float eps, float wd,
                                            float inv_bc1, float inv_sqrt_bc2) {
  float pe = pp[e], me = mm[e], ve = vv[e];
  adam_update(pe, g, me, ve, lr, beta1, beta2, eps, wd, inv_bc1, inv_sqrt_bc2);
  pp[e] = pe; mm[e] = me; vv[e] = ve;
}

// torch clip_grad_norm_: the factor that brings a gradient of squared norm normsq down to max_norm, at most 1
__device__ __forceinline__ float clip_coefficient(float normsq, float max_norm) {
  const float coef = max_norm / (sqrtf(normsq) + 1e-6f);
  return coef < 1.0f ? coef : 1.0f;
}

// The workgroup's sum of `local`, valid in thread 0: wave sums, then the waves in a FIXED order that is part of the result's bits --
// pairwise for the 256-thread kernels, left to right in thread 0 for the 1024-thread ones (one loop cannot give both orders).
template <int THREADS>
__device__ __forceinline__ float block_sum(float local) {
  static_assert(THREADS == 256 || THREADS == 1024, "an order of addition is defined for 4 and for 16 waves");
  __shared__ float part[THREADS / 64];
  local = wave_sum(local);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = local;
  __syncthreads();
  if (THREADS == 256) return (part[0] + part[1]) + (part[2] + part[3]);
  float sum = 0.0f;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) sum += part[w];
  }
  return sum;
}

// ... and on into normsq[0]: one partial per workgroup, summed in workgroup order by the last one to finish (common.h::ordered_block_sum):
// the same bits on every run and on every data-parallel replica -- the clip coefficient derived from it must not differ between ranks.
// normsq: NERF_NORMSQ_WS_FLOATS floats -- [0] the squared norm, then the ordered sum's workspace (tickets, one partial per workgroup)
template <int THREADS>
__device__ __forceinline__ void block_sum_into(float local, float* __restrict__ normsq, bool accumulate = true) {
  const float val[1] = {block_sum<THREADS>(local)};
  float* const out[1] = {normsq};
  ordered_block_sum<1>(val, out, reinterpret_cast<unsigned*>(normsq + 1), accumulate);
}

// 16-byte accesses on the 4-aligned body, scalar tail; VEC = false when a base pointer is not 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void adam_sweep(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, int64_t n, float gs, float lr, float beta1, float beta2,
                                           float eps, float wd, float inv_bc1, float inv_sqrt_bc2, _Float16* __restrict__ shadow = nullptr) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = VEC ? n / 4 : 0;
  for (int64_t i = tid; i < n4; i += stride) {
    f4 pp = load4<true>(p, i, n), mm = load4<true>(m, i, n), vv = load4<true>(v, i, n);
    const f4 gg = load4<true>(g, i, n);
#pragma unroll
    for (int e = 0; e < 4; ++e) adam_update(pp, e, gg[e] * gs, mm, vv, lr, beta1, beta2, eps, wd, inv_bc1, inv_sqrt_bc2);
    store4<true>(m, i, n, mm); store4<true>(v, i, n, vv); store4<true>(p, i, n, pp);
    store_shadow4<true>(shadow, i, n, pp);
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += stride) {
    adam_update(p[i], g[i] * gs, m[i], v[i], lr, beta1, beta2, eps, wd, inv_bc1, inv_sqrt_bc2);
    if (shadow != nullptr) shadow[i] = (_Float16)p[i];
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256)
adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
            float* __restrict__ v, int64_t n, float lr, float beta1, float beta2, float eps, float wd,
            float inv_bc1, float inv_sqrt_bc2, const float* __restrict__ grad_scale) {
  adam_sweep<VEC>(p, g, m, v, n, grad_scale ? *grad_scale : 1.0f, lr, beta1, beta2, eps, wd, inv_bc1, inv_sqrt_bc2);
}

// ---------------------------------------------------------------------------------------------
// Fused regulariser + clip + AdamW for flat hash-table parameters (replaces the
// torch sequence of reference run.py:611-630: TV-L1 over the flat vector, loss.backward() of it,
// clip_grad_norm_(max_norm) and AdamW.step()).  Two streaming passes:
//   pass 1  g_i += w/(n-1) * (sign(p_i - p_{i-1}) - sign(p_{i+1} - p_i));  normsq += g_i^2
//   pass 2  AdamW with g * min(1, max_norm / (sqrt(normsq) + 1e-6))
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float sgn(float x) { return (x > 0.0f) - (x < 0.0f); }

__device__ __forceinline__ float tv_term(float prev, float cur, float next, bool has_prev, bool has_next) {
  float t = 0.0f;
  if (has_prev) t += sgn(cur - prev);          // d/dp_i |p_i - p_{i-1}|
  if (has_next) t -= sgn(next - cur);          // d/dp_i |p_{i+1} - p_i|
  return t;
}

// the vector is up to four tables of seg elements back to back (Part 4's three deformation grids in one launch): the total
// variation does not couple the last element of a table with the first of the next.  starts(e): e is the first element of a table
struct TableStarts {
  int64_t seg;
  __device__ __forceinline__ bool operator()(int64_t e) const { return e == 0 || e == seg || e == 2 * seg || e == 3 * seg; }
};

template <bool VEC>
__global__ void __launch_bounds__(256)
tv_normsq_kernel(const float* __restrict__ p, float* __restrict__ g, int64_t n, float tv_scale, float grad_scale,
                 float* __restrict__ normsq, int64_t seg) {
  const TableStarts starts{seg};
  // grad_scale (1/world after a summing all-reduce) applies to the DATA gradient only: the TV term is
  // a function of the replicated parameters and must not be divided by the world size
  const bool rewrite = tv_scale != 0.0f || grad_scale != 1.0f;
  float local = 0.0f;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = VEC ? n / 4 : 0;
  for (int64_t i = tid; i < n4; i += stride) {
    f4 gg = reinterpret_cast<f4*>(g)[i];
    gg[0] *= grad_scale; gg[1] *= grad_scale; gg[2] *= grad_scale; gg[3] *= grad_scale;
    if (tv_scale != 0.0f) {
      const f4 pp = reinterpret_cast<const f4*>(p)[i];
      const int64_t e0 = 4 * i;
      const bool has_prev = !starts(e0), has_next = e0 + 4 < n && !starts(e0 + 4);   // seg is a multiple of 4 on this path
      const float before = has_prev ? p[e0 - 1] : 0.0f, after = has_next ? p[e0 + 4] : 0.0f;
      gg[0] += tv_scale * tv_term(before, pp[0], pp[1], has_prev, true);
      gg[1] += tv_scale * tv_term(pp[0], pp[1], pp[2], true, true);
      gg[2] += tv_scale * tv_term(pp[1], pp[2], pp[3], true, true);
      gg[3] += tv_scale * tv_term(pp[2], pp[3], after, true, has_next);
    }
    if (rewrite) reinterpret_cast<f4*>(g)[i] = gg;
    local += gg[0] * gg[0] + gg[1] * gg[1] + gg[2] * gg[2] + gg[3] * gg[3];
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += stride) {
    float gi = g[i] * grad_scale;
    if (tv_scale != 0.0f) {
      const bool has_prev = !starts(i), has_next = i + 1 < n && !starts(i + 1);
      gi += tv_scale * tv_term(has_prev ? p[i - 1] : 0.0f, p[i], has_next ? p[i + 1] : 0.0f, has_prev, has_next);
    }
    if (rewrite) g[i] = gi;
    local += gi * gi;
  }
  block_sum_into<256>(local, normsq);
}

template <bool VEC>
__global__ void __launch_bounds__(256)
adamw_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                  int64_t n, float lr, float beta1, float beta2, float eps, float wd, float inv_bc1,
                  float inv_sqrt_bc2, const float* __restrict__ normsq, float max_norm, float extra_scale,
                  _Float16* __restrict__ shadow) {
  float gs = extra_scale;
  if (normsq != nullptr && max_norm > 0.0f) gs *= clip_coefficient(*normsq * extra_scale * extra_scale, max_norm);
  adam_sweep<VEC>(p, g, m, v, n, gs, lr, beta1, beta2, eps, wd, inv_bc1, inv_sqrt_bc2, shadow);
}

// ---- the same two passes WITHOUT rewriting the gradient (38.5 instead of 42 bytes per parameter) --------------------------
// pass 1 leaves, instead of g + TV term (4 bytes written, 4 read back), the SIGNS it is made of: code_i = 1 + sign(p[i+1] - p[i])
// in two bits (0 behind the last element of a table), four elements per byte; the TV term of element i is
// tv_scale * (s[i-1] - s[i]).  Pass 2 rebuilds g * grad_scale + TV term from the codes -- from the OLD parameters' signs, whatever
// its neighbours have already written.
__device__ __forceinline__ unsigned tv_encode(int s, int e) { return (unsigned)(s + 1) << (2 * e); }       // sign s of element e of a byte
__device__ __forceinline__ int tv_decode(unsigned byte, int e) { return (int)((byte >> (2 * e)) & 3u) - 1; }

// the gradient both passes agree on: the scaled data gradient + the TV term from the signs before and behind the element
__device__ __forceinline__ float tv_gradient(float g, float grad_scale, float tv_scale, int s_prev, int s_cur) {
  return g * grad_scale + tv_scale * (float)(s_prev - s_cur);
}

// generic form (any alignment, any n): one chunk of four elements per thread and round
__global__ void __launch_bounds__(256)
tv_normsq_codes_kernel(const float* __restrict__ p, const float* __restrict__ g, int64_t n, float tv_scale, float grad_scale,
                       float* __restrict__ normsq, int64_t seg, uint8_t* __restrict__ codes, int accumulate) {
  const TableStarts starts{seg};
  float local = 0.0f;
  const int64_t n4 = (n + 3) / 4;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n4; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = 4 * q;
    float pp[6], gg[4];                        // pp[0] = p[e0-1] ... pp[5] = p[e0+4]
#pragma unroll
    for (int e = 0; e < 4; ++e) { pp[1 + e] = e0 + e < n ? p[e0 + e] : 0.0f; gg[e] = e0 + e < n ? g[e0 + e] : 0.0f; }
    if (tv_scale != 0.0f) {
      pp[0] = e0 > 0 ? p[e0 - 1] : 0.0f;
      pp[5] = e0 + 4 < n ? p[e0 + 4] : 0.0f;
      unsigned byte = 0;
      int s_prev = !starts(e0) ? (int)sgn(pp[1] - pp[0]) : 0;      // s[e0-1]: 0 across a seam
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t i = e0 + e;
        const int s_cur = (i + 1 < n && !starts(i + 1)) ? (int)sgn(pp[2 + e] - pp[1 + e]) : 0;
        if (i < n) {
          const float gi = tv_gradient(gg[e], grad_scale, tv_scale, s_prev, s_cur);
          local += gi * gi;
          byte |= tv_encode(s_cur, e);
        }
        s_prev = s_cur;
      }
      codes[q] = (uint8_t)byte;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float gi = gg[e] * grad_scale; local += gi * gi; }     // elements past n are zero
    }
  }
  block_sum_into<256>(local, normsq, accumulate != 0);
}

// the tables' form: 16-byte aligned, n a multiple of 4 and below 2^31.  kU chunks per thread and round, every load issued before the
// first is used and NO branch around a load (the neighbours p[e0-1], p[e0+4] come from clamped addresses; a table seam can only lie on
// a chunk's border since seg is a multiple of 4: two 32-bit seam tests per chunk).  The generic form above spent its time on 64-bit
// seam tests per element and on one chunk's two loads in flight per thread: 2.4 TB/s.
// 1024 threads per workgroup, at most one workgroup per CU: every workgroup ends with a same-address ticket atomic, and those
// retire one after the other (~20 ns each: 1024 workgroups of 256 spent 20 us of an 80-us launch queueing there; 4096: 60 us)
constexpr int kTvFastThreads = 1024;
template <bool TV>
__global__ void __launch_bounds__(kTvFastThreads)
tv_normsq_codes_fast_kernel(const float* __restrict__ p, const float* __restrict__ g, int n4, float tv_scale, float grad_scale,
                            float* __restrict__ normsq, int seam1, int seam2, int seam3, uint8_t* __restrict__ codes, int halo,
                            int accumulate) {
  // seam1..3: first element of the second, third and fourth table, -1 for a table that does not exist (computed on the host in
  // 64 bits: 2 * seg and 3 * seg do not fit an int for one table of 2^30 elements or more)
  // halo (a PIECE of one table: the sharded optimiser's slice): bit 0 -- p[-1] belongs to the same table, bit 1 -- p[n] does; the
  // piece's first TV term then reaches back to p[-1] (its sign is also left in codes[-1] for the AdamW pass), its last one on to p[n]
  constexpr int kU = 4;
  const f4* __restrict__ p4 = reinterpret_cast<const f4*>(p);
  const f4* __restrict__ g4 = reinterpret_cast<const f4*>(g);
  const int span = gridDim.x * blockDim.x, n = 4 * n4;
  float local = 0.0f;
  for (int q0 = blockIdx.x * blockDim.x + threadIdx.x; q0 < n4; q0 += kU * span) {
    f4 a[kU], b[kU];
    float lo[kU], hi[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int q = min(q0 + u * span, n4 - 1);           // past the end: the last chunk again (masked below)
      a[u] = p4[q];
      b[u] = g4[q];
      if (TV) {
        lo[u] = p[max(4 * q - 1, (halo & 1) ? -1 : 0)];
        hi[u] = p[min(4 * q + 4, (halo & 2) ? n : n - 1)];
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int q = q0 + u * span, e0 = 4 * q;
      if (q >= n4) break;
      float g0, g1, g2, g3;
      if (TV) {
        const bool first = (e0 == 0 && !(halo & 1)) || e0 == seam1 || e0 == seam2 || e0 == seam3;
        const int e4 = e0 + 4;
        const bool last = (e4 == n && !(halo & 2)) || (e4 != n && (e4 == seam1 || e4 == seam2 || e4 == seam3));
        const int s_in = first ? 0 : (int)sgn(a[u][0] - lo[u]), s0 = (int)sgn(a[u][1] - a[u][0]), s1 = (int)sgn(a[u][2] - a[u][1]),
                  s2 = (int)sgn(a[u][3] - a[u][2]), s3 = last ? 0 : (int)sgn(hi[u] - a[u][3]);
        g0 = tv_gradient(b[u][0], grad_scale, tv_scale, s_in, s0);
        g1 = tv_gradient(b[u][1], grad_scale, tv_scale, s0, s1);
        g2 = tv_gradient(b[u][2], grad_scale, tv_scale, s1, s2);
        g3 = tv_gradient(b[u][3], grad_scale, tv_scale, s2, s3);
        codes[q] = (uint8_t)(tv_encode(s0, 0) | tv_encode(s1, 1) | tv_encode(s2, 2) | tv_encode(s3, 3));
        // the sign the AdamW pass reads as the piece's s[-1]: the top code of the byte before the piece.  Its other three codes are kept:
        // where the pieces of one table share one code buffer they belong to the piece before (same stream: whichever ran last leaves the
        // same top code)
        if (q == 0 && (halo & 1)) codes[-1] = (uint8_t)((codes[-1] & 0x3Fu) | tv_encode(s_in, 3));
      } else {
        g0 = b[u][0] * grad_scale; g1 = b[u][1] * grad_scale; g2 = b[u][2] * grad_scale; g3 = b[u][3] * grad_scale;
      }
      local += (g0 * g0 + g1 * g1) + (g2 * g2 + g3 * g3);
    }
  }
  block_sum_into<kTvFastThreads>(local, normsq, accumulate != 0);
}

// One small parameter group (a tiny MLP's few thousand weights) in ONE launch: squared norm of the scaled gradient, clip coefficient,
// AdamW -- instead of a zeroing launch, a norm launch and an AdamW launch of ~4.5 us each for 45 KB of data.  EVERY workgroup sums
// the whole gradient itself (threads in a fixed stride, waves in order: the same bits in every workgroup and every run -- the vector
// sits in L2) and then steps its own kSmallOptThreads elements: no exchange between workgroups, one element per thread in the update.
// zero_grads: the gradient is left zeroed for the next step's accumulating backward (not while other workgroups may still read it:
// only with one workgroup, i.e. n <= kSmallOptThreads -- the launcher falls back to a memset otherwise).
constexpr int kSmallOptThreads = 1024;
__global__ void __launch_bounds__(kSmallOptThreads)
clip_adamw_small_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int n, float lr,
                        float beta1, float beta2, float eps, float wd, float inv_bc1, float inv_sqrt_bc2, float max_norm, float grad_scale,
                        float* __restrict__ normsq_out, int zero_grads) {
  float local = 0.0f;
  for (int i = threadIdx.x; i < n; i += kSmallOptThreads) { const float gi = g[i] * grad_scale; local += gi * gi; }
  __shared__ float total;
  const float sum = block_sum<kSmallOptThreads>(local);
  if (threadIdx.x == 0) {
    total = sum;
    if (normsq_out != nullptr && blockIdx.x == 0) *normsq_out = sum;
  }
  __syncthreads();
  const float clip = max_norm > 0.0f ? clip_coefficient(total, max_norm) : 1.0f;
  const int i = blockIdx.x * kSmallOptThreads + threadIdx.x;
  if (i < n) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam_update(pp, g[i] * grad_scale * clip, mm, vv, lr, beta1, beta2, eps, wd, inv_bc1, inv_sqrt_bc2);
    p[i] = pp; m[i] = mm; v[i] = vv;
    if (zero_grads) g[i] = 0.0f;
  }
}

__global__ void __launch_bounds__(256)
adamw_clip_tv_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                     float lr, float beta1, float beta2, float eps, float wd, float inv_bc1, float inv_sqrt_bc2,
                     const float* __restrict__ normsq, float max_norm, float grad_scale, const uint8_t* __restrict__ codes,
                     int64_t tv_split, float tv_scale_lo, float tv_scale_hi, _Float16* __restrict__ shadow, int vec,
                     int64_t lr_split, float lr_hi, int halo_lo) {
  const float clip = normsq != nullptr && max_norm > 0.0f ? clip_coefficient(*normsq, max_norm) : 1.0f;   // of the scaled gradient + TV term
  const int64_t n4 = (n + 3) / 4;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < n4; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = 4 * q;
    const bool whole = vec && e0 + 4 <= n;
    f4 pp, gg, mm, vv;
    if (whole) { pp = load4<true>(p, q, n); gg = load4<true>(g, q, n); mm = load4<true>(m, q, n); vv = load4<true>(v, q, n); }
    else { pp = load4<false>(p, q, n); gg = load4<false>(g, q, n); mm = load4<false>(m, q, n); vv = load4<false>(v, q, n); }
    int s_prev = 0;
    unsigned byte = tv_encode(0, 0) | tv_encode(0, 1) | tv_encode(0, 2) | tv_encode(0, 3);      // no codes: every sign 0
    if (codes != nullptr) {
      byte = codes[q];
      // THE SEAM RULE of this kernel: s[e0-1] is the top code of the byte before, and 0 only in front of the first chunk (halo_lo: a
      // piece inside a table, codes[-1] holds s[-1]).  Pass 1 leaves sign 0 behind the last element of every table, so a seam needs
      // no test here -- except that the chunk at e0 == tv_split reads a byte of the LOWER range, which pass 1 never wrote when
      // tv_scale_lo == 0: the open ADVICE.md finding on this kernel ("takes s_prev of the chunk at e0 == tv_split from codes[q-1]").
      // Its fix belongs in this condition (`&& e0 != tv_split`); behaviour is kept as it was until then
      s_prev = (q > 0 || halo_lo) ? tv_decode(codes[q - 1], 3) : 0;
    }
    const float tv_scale = e0 < tv_split ? tv_scale_lo : tv_scale_hi;       // the splits are multiples of 4: one choice per chunk
    const float lr_q = e0 < lr_split ? lr : lr_hi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int s_cur = tv_decode(byte, e);
      adam_update(pp, e, tv_gradient(gg[e], grad_scale, tv_scale, s_prev, s_cur) * clip, mm, vv, lr_q, beta1, beta2, eps, wd, inv_bc1, inv_sqrt_bc2);
      s_prev = s_cur;
    }
    if (whole) { store4<true>(m, q, n, mm); store4<true>(v, q, n, vv); store4<true>(p, q, n, pp); store_shadow4<true>(shadow, q, n, pp); }
    else { store4<false>(m, q, n, mm); store4<false>(v, q, n, vv); store4<false>(p, q, n, pp); store_shadow4<false>(shadow, q, n, pp); }
  }
}

__global__ void __launch_bounds__(256) f32_to_f16_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (_Float16)src[i];
}

// ---- what the entries below share on the host side ----
static bool aligned16(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

struct BiasCorrection {                  // Adam's 1 / (1 - beta1^step) and 1 / sqrt(1 - beta2^step), formed in double
  float inv_bc1, inv_sqrt_bc2;
  BiasCorrection(float beta1, float beta2, int step)
      : inv_bc1((float)(1.0 / (1.0 - pow((double)beta1, step)))), inv_sqrt_bc2((float)(1.0 / sqrt(1.0 - pow((double)beta2, step)))) {}
};

// workgroups of 256 threads for a grid-stride sweep over work_items (+ extra), at most cap
static int stream_blocks(int64_t work_items, int64_t cap, int extra = 0) {
  const int64_t blocks = (work_items + 255) / 256 + extra;
  return (int)(blocks < cap ? blocks : cap);
}

// launch(std::true_type / std::false_type): one spelling of a launch whose kernel has a bool template parameter
template <class Launch>
static void with_flag(bool flag, Launch launch) {
  if (flag) launch(std::true_type{});
  else launch(std::false_type{});
}

// nothing to add: a storing call still leaves the norm defined
static int empty_normsq(const char* what, float* normsq_dev, int accumulate, nerf_stream_t stream) {
  if (!accumulate && hipMemsetAsync(normsq_dev, 0, sizeof(float), as_stream(stream)) != hipSuccess) return fail(NERF_ELAUNCH, "%s: memset failed", what);
  return NERF_OK;
}

static float tv_scale_of(float tv_weight, int64_t table_elems) {      // d/dp of mean|p[1:] - p[:-1]| * w, per table
  return table_elems > 1 ? tv_weight / (float)(table_elems - 1) : 0.0f;
}

// tv_normsq_codes_fast_kernel over n elements (16-byte aligned, n a multiple of 4 and below 2^31); seam: the kernel's seam1..3.
// block_cap: the most workgroups (option tv_blocks), anything outside 1..4096 for one per CU
static void launch_tv_codes_fast(const float* params, const float* grads, int64_t n, float tv_scale, float grad_scale, float* normsq_dev,
                                 const int (&seam)[3], void* tv_codes, int halo, int accumulate, int64_t block_cap, nerf_stream_t stream) {
  int n_cu = 256;
  (void)device_cu_count(&n_cu);
  if (block_cap < 1 || block_cap > 4096) block_cap = n_cu;
  const int64_t blocks = (n / 4 + 4 * kTvFastThreads - 1) / (4 * kTvFastThreads);          // four chunks per thread and round
  with_flag(tv_scale != 0.0f, [&](auto tv) {
    hipLaunchKernelGGL(tv_normsq_codes_fast_kernel<decltype(tv)::value>, dim3((int)(blocks < block_cap ? blocks : block_cap)), dim3(kTvFastThreads),
                       0, as_stream(stream), params, grads, (int)(n / 4), tv_scale, grad_scale, normsq_dev, seam[0], seam[1], seam[2],
                       static_cast<uint8_t*>(tv_codes), decltype(tv)::value ? halo : 0, accumulate);
  });
}

// adamw_clip_tv_kernel for the entry `what`, which has checked n, step and its splits
static int launch_adamw_clip_tv(const char* what, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                                float lr, float beta1, float beta2, float eps, float weight_decay, const float* normsq_dev, float max_norm,
                                float grad_scale, const void* tv_codes, int64_t tv_split, float tv_scale_lo, float tv_scale_hi,
                                void* params_f16_out, int64_t lr_split, float lr_hi, int halo_lo, nerf_stream_t stream) {
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(params && grads && exp_avg && exp_avg_sq, "%s: NULL pointer", what);
  NERF_REQUIRE(params_f16_out == nullptr || ((uintptr_t)params_f16_out & 7) == 0, "%s: params_f16_out unaligned", what);
  const BiasCorrection bc(beta1, beta2, step);
  hipLaunchKernelGGL(adamw_clip_tv_kernel, dim3(stream_blocks((n + 3) / 4, 4096)), dim3(256), 0, as_stream(stream), params, grads, exp_avg,
                     exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc.inv_bc1, bc.inv_sqrt_bc2, normsq_dev, max_norm, grad_scale,
                     static_cast<const uint8_t*>(tv_codes), tv_split, tv_scale_lo, tv_scale_hi, static_cast<_Float16*>(params_f16_out),
                     (int)aligned16(params, grads, exp_avg, exp_avg_sq), lr_split, lr_hi, halo_lo);
  return check_launch(what);
}

}  // namespace nerf

extern "C" int nerf_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                              int64_t n, int step, float lr, float beta1, float beta2, float eps,
                              float weight_decay, const float* grad_scale_dev, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && step >= 1, "nerf_adam_step: n=%lld step=%d", (long long)n, step);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(params && grads && exp_avg && exp_avg_sq, "nerf_adam_step: NULL pointer");
  const nerf::BiasCorrection bc(beta1, beta2, step);
  nerf::with_flag(nerf::aligned16(params, grads, exp_avg, exp_avg_sq), [&](auto vec) {
    hipLaunchKernelGGL(nerf::adam_kernel<decltype(vec)::value>, dim3(nerf::stream_blocks(n / 4, 2048, 1)), dim3(256), 0, nerf::as_stream(stream),
                       params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc.inv_bc1, bc.inv_sqrt_bc2, grad_scale_dev);
  });
  return nerf::check_launch("nerf_adam_step");
}

// ---- the gradient-REWRITING passes: nerf_tv_normsq and its siblings answer under its name, as do nerf_adamw_clip_step's ----
static int tv_normsq_impl(const float* params, float* grads, int64_t n, float tv_weight, float grad_scale,
                          float* normsq_dev, bool zero_first, nerf_stream_t stream, int n_tables = 1) {
  NERF_REQUIRE(n >= 0 && normsq_dev && n_tables >= 1 && n_tables <= 4 && n % n_tables == 0, "nerf_tv_normsq: bad arguments");
  const int64_t seg = n / n_tables;
  NERF_REQUIRE(n_tables == 1 || seg % 4 == 0, "nerf_tv_normsq_accum_tables: %lld elements per table (a multiple of 4)", (long long)seg);
  if (zero_first && hipMemsetAsync(normsq_dev, 0, sizeof(float) * (1 + nerf::kOrderedSumTickets), nerf::as_stream(stream)) != hipSuccess)   // the norm and the tickets
    return nerf::fail(NERF_ELAUNCH, "nerf_tv_normsq: memset failed");
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(params && grads, "nerf_tv_normsq: NULL pointer");
  static_assert(NERF_NORMSQ_WS_FLOATS >= 1 + nerf::kOrderedSumTickets + 4096, "the norm, the tickets, one partial per workgroup");
  // 1024: measured -- 512 +6 %, 256 +50 %, 2048 +15 % (one same-address atomic per workgroup against HBM streams in flight)
  nerf::with_flag(nerf::aligned16(params, grads), [&](auto vec) {
    hipLaunchKernelGGL(nerf::tv_normsq_kernel<decltype(vec)::value>, dim3(nerf::stream_blocks(n / 4, 1024, 1)), dim3(256), 0, nerf::as_stream(stream),
                       params, grads, n, nerf::tv_scale_of(tv_weight, seg), grad_scale, normsq_dev, seg);
  });
  return nerf::check_launch("nerf_tv_normsq");
}

extern "C" int nerf_tv_normsq(const float* params, float* grads, int64_t n, float tv_weight, float grad_scale,
                              float* normsq_dev, nerf_stream_t stream) {
  return tv_normsq_impl(params, grads, n, tv_weight, grad_scale, normsq_dev, true, stream);
}

extern "C" int nerf_tv_normsq_accum(const float* params, float* grads, int64_t n, float tv_weight, float grad_scale,
                                    float* normsq_dev, nerf_stream_t stream) {
  return tv_normsq_impl(params, grads, n, tv_weight, grad_scale, normsq_dev, false, stream);
}

extern "C" int nerf_tv_normsq_accum_tables(const float* params, float* grads, int64_t n, int n_tables, float tv_weight,
                                           float grad_scale, float* normsq_dev, nerf_stream_t stream) {
  return tv_normsq_impl(params, grads, n, tv_weight, grad_scale, normsq_dev, false, stream, n_tables);
}

static int adamw_clip_impl(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                           int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                           const float* normsq_dev, float max_norm, float grad_scale, void* shadow_f16, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && step >= 1, "nerf_adamw_clip_step: n=%lld step=%d", (long long)n, step);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(params && grads && exp_avg && exp_avg_sq, "nerf_adamw_clip_step: NULL pointer");
  const nerf::BiasCorrection bc(beta1, beta2, step);
  nerf::with_flag(nerf::aligned16(params, grads, exp_avg, exp_avg_sq), [&](auto vec) {
    hipLaunchKernelGGL(nerf::adamw_clip_kernel<decltype(vec)::value>, dim3(nerf::stream_blocks(n / 4, 4096, 1)), dim3(256), 0, nerf::as_stream(stream),
                       params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc.inv_bc1, bc.inv_sqrt_bc2, normsq_dev,
                       max_norm, grad_scale, static_cast<_Float16*>(shadow_f16));
  });
  return nerf::check_launch("nerf_adamw_clip_step");
}

extern "C" int nerf_adamw_clip_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                    int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                    const float* normsq_dev, float max_norm, float grad_scale, nerf_stream_t stream) {
  return adamw_clip_impl(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay, normsq_dev, max_norm,
                         grad_scale, nullptr, stream);
}

extern "C" int nerf_adamw_clip_step_shadow(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                           int step, float lr, float beta1, float beta2, float eps, float weight_decay,
                                           const float* normsq_dev, float max_norm, float grad_scale, void* params_f16_out,
                                           nerf_stream_t stream) {
  NERF_REQUIRE(params_f16_out != nullptr && ((uintptr_t)params_f16_out & 7) == 0, "nerf_adamw_clip_step_shadow: params_f16_out NULL or unaligned");
  return adamw_clip_impl(params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay, normsq_dev, max_norm,
                         grad_scale, params_f16_out, stream);
}

extern "C" int nerf_f32_to_f16(const float* src, void* dst_f16, int64_t n, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0, "nerf_f32_to_f16: n=%lld", (long long)n);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(src && dst_f16, "nerf_f32_to_f16: NULL pointer");
  hipLaunchKernelGGL(nerf::f32_to_f16_kernel, dim3(nerf::stream_blocks(n, 4096)), dim3(256), 0, nerf::as_stream(stream), src,
                     static_cast<_Float16*>(dst_f16), n);
  return nerf::check_launch("nerf_f32_to_f16");
}

// ---- TV + norm and clip + AdamW without the gradient rewrite (see tv_normsq_codes_kernel) ----
extern "C" size_t nerf_tv_codes_bytes(int64_t n) { return n > 0 ? (size_t)((n + 3) / 4) : 0; }

extern "C" int nerf_tv_normsq_codes(const float* params, const float* grads, int64_t n, int n_tables, float tv_weight, float grad_scale,
                                    float* normsq_dev, int accumulate, void* tv_codes, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && normsq_dev && n_tables >= 1 && n_tables <= 4 && n % n_tables == 0, "nerf_tv_normsq_codes: bad arguments");
  if (n == 0) return nerf::empty_normsq("nerf_tv_normsq_codes", normsq_dev, accumulate, stream);
  const int64_t seg = n / n_tables;
  NERF_REQUIRE(n_tables == 1 || seg % 4 == 0, "nerf_tv_normsq_codes: %lld elements per table (a multiple of 4)", (long long)seg);
  NERF_REQUIRE(params && grads && (tv_weight == 0.0f || tv_codes), "nerf_tv_normsq_codes: NULL pointer");
  const float tv_scale = nerf::tv_scale_of(tv_weight, seg);
  if (nerf::aligned16(params, grads) && n % 4 == 0 && n < ((int64_t)1 << 31) - 16) {
    int seam[3];                            // k * seg < n < 2^31 for every table k that exists
    for (int k = 1; k <= 3; ++k) seam[k - 1] = k < n_tables ? (int)(k * seg) : -1;
    nerf::launch_tv_codes_fast(params, grads, n, tv_scale, grad_scale, normsq_dev, seam, tv_codes, 0, accumulate, nerf::options().tv_blocks, stream);
  } else {        // generic form; 1024: its partials fit NERF_NORMSQ_WS_FLOATS
    hipLaunchKernelGGL(nerf::tv_normsq_codes_kernel, dim3(nerf::stream_blocks((n + 3) / 4, 1024)), dim3(256), 0, nerf::as_stream(stream), params,
                       grads, n, tv_scale, grad_scale, normsq_dev, seg, static_cast<uint8_t*>(tv_codes), accumulate);
  }
  return nerf::check_launch("nerf_tv_normsq_codes");
}

extern "C" int nerf_adamw_clip_step_tv(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr,
                                       float beta1, float beta2, float eps, float weight_decay, const float* normsq_dev, float max_norm,
                                       float grad_scale, const void* tv_codes, int64_t tv_split, float tv_weight_lo, int64_t seg_lo,
                                       float tv_weight_hi, int64_t seg_hi, int64_t lr_split, float lr_hi, void* params_f16_out,
                                       nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && step >= 1 && tv_split >= 0 && seg_lo >= 0 && seg_hi >= 0, "nerf_adamw_clip_step_tv: n=%lld step=%d", (long long)n, step);
  NERF_REQUIRE((tv_split % 4 == 0 || tv_split >= n) && (lr_split % 4 == 0 || lr_split >= n),
               "nerf_adamw_clip_step_tv: tv_split / lr_split must be multiples of 4 (or past the end)");
  return nerf::launch_adamw_clip_tv("nerf_adamw_clip_step_tv", params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay,
                                    normsq_dev, max_norm, grad_scale, tv_codes, tv_split, tv_codes ? nerf::tv_scale_of(tv_weight_lo, seg_lo) : 0.0f,
                                    tv_codes ? nerf::tv_scale_of(tv_weight_hi, seg_hi) : 0.0f, params_f16_out, lr_split <= 0 ? n : lr_split, lr_hi,
                                    0, stream);
}

// ---- the same two passes on a PIECE [params, params + n) of ONE table of table_elems elements (the sharded optimiser of the
// data-parallel engines: every rank steps its slice of the flat table buffer).  halo bit 0: params[-1] belongs to the same table and
// holds its current value, bit 1: params[n] does -- the TV terms at the piece's ends then equal the whole-table pass.  tv_codes points
// at the piece's first code byte inside a buffer that has at least one byte before it (codes[-1] receives the sign of
// params[0] - params[-1] in its top two bits; its other bits are kept).  n a multiple of 4, 16-byte aligned pointers.
extern "C" int nerf_tv_normsq_codes_piece(const float* params, const float* grads, int64_t n, int64_t table_elems, int halo, float tv_weight,
                                          float grad_scale, float* normsq_dev, int accumulate, void* tv_codes, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && normsq_dev && table_elems >= n && halo >= 0 && halo <= 3, "nerf_tv_normsq_codes_piece: bad arguments");
  if (n == 0) return nerf::empty_normsq("nerf_tv_normsq_codes_piece", normsq_dev, accumulate, stream);
  NERF_REQUIRE(params && grads && (tv_weight == 0.0f || tv_codes), "nerf_tv_normsq_codes_piece: NULL pointer");
  NERF_REQUIRE(nerf::aligned16(params, grads) && n % 4 == 0 && n < ((int64_t)1 << 31) - 16,
               "nerf_tv_normsq_codes_piece: 16-byte aligned pointers and n a multiple of 4");
  nerf::launch_tv_codes_fast(params, grads, n, nerf::tv_scale_of(tv_weight, table_elems), grad_scale, normsq_dev, {-1, -1, -1}, tv_codes, halo,
                             accumulate, 0, stream);        // one workgroup per CU: option tv_blocks is the whole-table entry's
  return nerf::check_launch("nerf_tv_normsq_codes_piece");
}

extern "C" int nerf_adamw_clip_step_tv_piece(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                                             float lr, float beta1, float beta2, float eps, float weight_decay, const float* normsq_dev,
                                             float max_norm, float grad_scale, const void* tv_codes, float tv_weight, int64_t table_elems,
                                             int halo_lo, void* params_f16_out, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && step >= 1 && table_elems >= n, "nerf_adamw_clip_step_tv_piece: n=%lld step=%d", (long long)n, step);
  const float sc = tv_codes ? nerf::tv_scale_of(tv_weight, table_elems) : 0.0f;
  return nerf::launch_adamw_clip_tv("nerf_adamw_clip_step_tv_piece", params, grads, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps,
                                    weight_decay, normsq_dev, max_norm, grad_scale, tv_codes, n, sc, sc, params_f16_out, n, lr,
                                    (tv_codes && halo_lo) ? 1 : 0, stream);
}

// ---- one small group (n <= 65536: a tiny MLP's weights) in ONE launch (n / 1024 workgroups, each summing the whole gradient itself):
// squared norm of grads * grad_scale (fixed order), global-norm clip, AdamW (clip_grad_norm_ + AdamW.step() of reference run.py:624-629 for
// the decoder group).  normsq_out (nullable) receives the squared norm; zero_grads: the gradient vector is left zeroed (the next backward adds).
extern "C" int nerf_clip_adamw_small(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, float max_norm, float grad_scale,
                                     float* normsq_out, int zero_grads, nerf_stream_t stream) {
  NERF_REQUIRE(n >= 0 && n <= 65536 && step >= 1, "nerf_clip_adamw_small: n=%lld (at most 65536) step=%d", (long long)n, step);
  if (n == 0) return NERF_OK;
  NERF_REQUIRE(params && grads && exp_avg && exp_avg_sq, "nerf_clip_adamw_small: NULL pointer");
  const nerf::BiasCorrection bc(beta1, beta2, step);
  const int blocks = (int)((n + nerf::kSmallOptThreads - 1) / nerf::kSmallOptThreads);
  hipLaunchKernelGGL(nerf::clip_adamw_small_kernel, dim3(blocks), dim3(nerf::kSmallOptThreads), 0, nerf::as_stream(stream), params, grads,
                     exp_avg, exp_avg_sq, (int)n, lr, beta1, beta2, eps, weight_decay, bc.inv_bc1, bc.inv_sqrt_bc2, max_norm,
                     grad_scale, normsq_out, (zero_grads && blocks == 1) ? 1 : 0);
  if (int rc = nerf::check_launch("nerf_clip_adamw_small"); rc != NERF_OK) return rc;
  if (zero_grads && blocks > 1 && hipMemsetAsync(grads, 0, sizeof(float) * (size_t)n, nerf::as_stream(stream)) != hipSuccess)
    return nerf::fail(NERF_ELAUNCH, "nerf_clip_adamw_small: memset failed");
  return NERF_OK;
}
