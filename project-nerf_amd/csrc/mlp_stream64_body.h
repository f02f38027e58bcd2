// The body of the 64-samples-per-wave inference kernel (mlp_fwd.hip), included INSIDE a kernel that has `a` (FwdArgs, const) and
// `smem` (the dynamic LDS) in scope: mlp_fwd_stream64_kernel and its counted twin share this text.  It is text and not a
// __device__ __forceinline__ function on purpose: a callee is optimised on its own before it is inlined, so the body then passes the
// simplification pipeline twice and mlp_fwd_stream64_kernel compiles differently (15463 -> 15472 instructions with the arguments
// by reference, by value or as scalars alike) -- included as text, the kernel is the compiler's same code.
  float* bias_lds = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, q = lane >> 4;

  const float* bias_g = reinterpret_cast<const float*>(a.packed + kPackBiasOff);
  for (int i = tid; i < kBiasFloats; i += kChain64Threads) bias_lds[i] = bias_g[i];

  // chunks 0 and 1 into ring slots 0 and 1: four waves, 1 KiB per wave and piece (the tail pieces read into the stream's padding)
  const char* src = a.packed + kPackFwd16Off;
  char* ring = smem + kBiasLdsBytes;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int frag0 = plan::kFwdChunks.chunk_frag0[c], count = plan::kFwdChunks.chunk_count[c];
    for (int i = 0; i < (count + 3) / 4; ++i)
      __builtin_amdgcn_global_load_lds((gptr_t)(src + (size_t)(frag0 + wave + 4 * i) * 1024 + lane * 16),
                                       (lptr_t)(ring + c * kRingSlotBytes + (wave + 4 * i) * 1024), 16, 0, 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const unsigned bb = lds_addr(smem) + 16u * q;
  const unsigned ab0 = lds_addr(ring) + 16u * lane, ab1 = ab0 + kRingSlotBytes;
  const unsigned ldsw = __builtin_amdgcn_readfirstlane(lds_addr(ring) + 1024u * wave);
  const unsigned voff = 1024u * wave + 16u * lane;

  float psc[2][8], pph[2][8], dsc[1][8], dph[1][8];          // scale and phase of this lane's features: loop-invariant
  fourier_lane_constants<2, kPosDim>(q, psc, pph);
  fourier_lane_constants<1, kDirDim>(q, dsc, dph);
  const int64_t n_tiles = (a.n + kTileSamples - 1) / kTileSamples;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t n0 = tile * kTileSamples + wave * 64 + c16;
    bf16x8 xenc[8], denc[4];      // x[4 kk + g], d[g]
    int64_t nn[4];
    bool live[4];
    // ray mode with a sample count that is a multiple of 64: the wave's 64 samples lie on ONE ray -- its origin, direction and the
    // direction's code once per tile instead of once per sample half (an integer division, a square root and three divisions each)
    const bool one_ray = a.n_samples > 0 && (a.n_samples & 63) == 0;
    float ro[3] = {0.f, 0.f, 0.f}, rd[3] = {0.f, 0.f, 0.f};
    bf16x8 de_ray[1];
    if (one_ray) {
      const int64_t first = n0 - c16 < a.n ? n0 - c16 : a.n - 1;
      const int64_t ray = (uint32_t)first / (uint32_t)a.n_samples;
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) { ro[c] = a.rays_o[ray * 3 + c]; rd[c] = a.rays_d[ray * 3 + c]; }
      const float nrm = sqrtf(add_rn(add_rn(mul_rn(rd[0], rd[0]), mul_rn(rd[1], rd[1])), mul_rn(rd[2], rd[2])));
      v[0] = rd[0] / nrm; v[1] = rd[1] / nrm; v[2] = rd[2] / nrm;
      fourier_operand16_hoisted<1, kDirDim>(v[0], v[1], v[2], q, dsc, dph, de_ray);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      nn[g] = n0 + 16 * g;
      live[g] = nn[g] < a.n;
      const int64_t nc = live[g] ? nn[g] : a.n - 1;
      bf16x8 xe[2], de[1];
      if (a.n_samples < 0) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int f = 32 * kk + 8 * q + j;
            xe[kk][j] = (__bf16)(f < kPosDim ? a.rays_o[nc * kPosDim + f] : (f == kPosDim ? 1.0f : 0.0f));
          }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int f = 8 * q + j;
          de[0][j] = (__bf16)(f < kDirDim ? a.rays_d[nc * kDirDim + f] : (f == kDirDim ? 1.0f : 0.0f));
        }
      } else if (one_ray) {
        const float zz = a.z[nc];
        fourier_operand16_hoisted<2, kPosDim>(add_rn(ro[0], mul_rn(rd[0], zz)), add_rn(ro[1], mul_rn(rd[1], zz)),
                                              add_rn(ro[2], mul_rn(rd[2], zz)), q, psc, pph, xe);
        de[0] = de_ray[0];
      } else {
        float p[3], v[3];
        sample_geometry(a, nc, p, v);
        fourier_operand16_hoisted<2, kPosDim>(p[0], p[1], p[2], q, psc, pph, xe);
        fourier_operand16_hoisted<1, kDirDim>(v[0], v[1], v[2], q, dsc, dph, de);
      }
      xenc[0 + g] = xe[0];
      xenc[4 + g] = xe[1];
      denc[g] = de[0];
    }
    float sg[4], col[12];
    fwd_stream64_pass(ab0, ab1, bb, xenc, denc, src, voff, ldsw, sg, col);
    if (q == 0) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (live[g]) {
          a.sigma[nn[g]] = fmaxf(sg[g], 0.0f);
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) a.rgb[nn[g] * 3 + ch] = 1.0f / (1.0f + __expf(-col[3 * g + ch]));
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last pass's look-ahead DMA must not outlive the wave
