// Occupancy-grid refresh helpers (reference src/renderer.py:35-132):
// lattice generation and the overwrite / running-max + threshold + active count pass.
#include "common.h"
#include "lattice.h"

namespace nerf {

__global__ void __launch_bounds__(256)
lattice_kernel(float bound, int res, float step, float* __restrict__ out) {
  const int64_t total = (int64_t)res * res * res;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    const int iz = (int)(g % res), iy = (int)((g / res) % res), ix = (int)(g / ((int64_t)res * res));
    out[g * 3 + 0] = lattice_node(ix, res, bound, step);   // 'ij' meshgrid, x slowest (renderer.py:53-54)
    out[g * 3 + 1] = lattice_node(iy, res, bound, step);
    out[g * 3 + 2] = lattice_node(iz, res, bound, step);
  }
}

__global__ void __launch_bounds__(256)
grid_update_kernel(const float* __restrict__ cur, float* __restrict__ grid, uint8_t* __restrict__ binary,
                   int64_t n, float decay, int dynamic, float threshold, unsigned long long* __restrict__ count) {
  unsigned long long local = 0;
  for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < n; g += (int64_t)gridDim.x * blockDim.x) {
    float v = cur[g];
    if (dynamic) v = fmaxf(grid[g] * decay, v);          // renderer.py:122-125
    grid[g] = v;
    const bool on = v > threshold;
    binary[g] = on ? 1 : 0;
    local += on ? 1 : 0;
  }
  // one atomic per wave
  for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(count, local);
}

}  // namespace nerf

using namespace nerf;

extern "C" int nerf_grid_lattice(float bound, int resolution, float* pts_out, nerf_stream_t stream) {
  NERF_REQUIRE(bound > 0.0f && resolution >= 2 && pts_out, "nerf_grid_lattice: bad arguments");
  const float step = lattice_step(bound, resolution);
  hipLaunchKernelGGL(lattice_kernel, dim3(2048), dim3(256), 0, as_stream(stream), bound, resolution, step, pts_out);
  return check_launch("nerf_grid_lattice");
}

extern "C" int nerf_grid_update(const float* sigma, float* grid, uint8_t* binary_grid, int64_t n_cells,
                                float decay, int dynamic, float threshold, unsigned long long* active_count,
                                nerf_stream_t stream) {
  NERF_REQUIRE(n_cells > 0 && sigma && grid && binary_grid && active_count, "nerf_grid_update: bad arguments");
  if (hipMemsetAsync(active_count, 0, sizeof(unsigned long long), as_stream(stream)) != hipSuccess)
    return fail(NERF_ELAUNCH, "nerf_grid_update: memset failed");
  int64_t blocks = (n_cells + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(grid_update_kernel, dim3((int)blocks), dim3(256), 0, as_stream(stream), sigma, grid, binary_grid,
                     n_cells, decay, dynamic, threshold, active_count);
  return check_launch("nerf_grid_update");
}

// ---- the Instant-NGP field's refresh as one launch chain (reference DensityGrid.update around the hash field,
// src/renderer.py:35-132, the density query src/decoders.py:148-153) ----
// clear the count -> per slab of `slab_cells` cells: hash gather (points from the cell index, or from `pts`) -> sigma-net chain
// with nerf_grid_update's fold in its epilogue.  The slabs share ONE operand image; stream order serialises them.  No lattice
// tensor, no rgb, no view directions, no allocation, no host read: 2 * ceil(n_cells / slab_cells) + 1 enqueues.
extern "C" size_t nerf_instant_grid_update_workspace_bytes(int64_t slab_cells) {
  if (slab_cells <= 0) return 0;
  const size_t rows = ((size_t)slab_cells + 127) / 128 * 128;
  return (rows * 32 * 2 + 255) / 256 * 256;
}

extern "C" int nerf_instant_grid_update(const void* packed, const float* table_f32, const void* table_f16, int n_levels,
                                        const float* scale_host, const unsigned* res_host, const unsigned* size_host,
                                        const unsigned* offset_host, const unsigned* dense_host, float hash_bound, const float* pts,
                                        int64_t n_cells, int resolution, float grid_bound, float* grid, uint8_t* binary_grid, float decay,
                                        int dynamic, float threshold, unsigned long long* active_count, int64_t slab_cells,
                                        void* workspace, nerf_stream_t stream) {
  NERF_REQUIRE(n_cells >= 0, "nerf_instant_grid_update: n_cells=%lld", (long long)n_cells);
  if (pts != nullptr) {
    NERF_REQUIRE(resolution == 0, "nerf_instant_grid_update: resolution=%d with a point buffer (must be 0)", resolution);
    if (n_cells == 0) return NERF_OK;
  } else {
    NERF_REQUIRE(resolution >= 2 && resolution <= 32768, "nerf_instant_grid_update: resolution=%d (2..32768)", resolution);
    NERF_REQUIRE(n_cells == (int64_t)resolution * resolution * resolution, "nerf_instant_grid_update: n_cells=%lld is not resolution^3 (%d)",
                 (long long)n_cells, resolution);
    NERF_REQUIRE(grid_bound > 0.0f, "nerf_instant_grid_update: grid_bound must be positive");
  }
  NERF_REQUIRE(n_levels == 16, "nerf_instant_grid_update: n_levels=%d (the default-shape sigma-net reads 16 levels x 2 features)", n_levels);
  NERF_REQUIRE((table_f32 == nullptr) != (table_f16 == nullptr), "nerf_instant_grid_update: exactly one of table_f32 / table_f16");
  NERF_REQUIRE(slab_cells > 0 && slab_cells % 128 == 0, "nerf_instant_grid_update: slab_cells=%lld (a positive multiple of 128)",
               (long long)slab_cells);
  NERF_REQUIRE(slab_cells * 32 < ((int64_t)1 << 31), "nerf_instant_grid_update: slab too large (slab_cells * 32 must stay below 2^31)");
  NERF_REQUIRE(hash_bound > 0.0f, "nerf_instant_grid_update: hash_bound must be positive");
  NERF_REQUIRE(packed && scale_host && res_host && size_host && offset_host && dense_host && grid && binary_grid && active_count && workspace,
               "nerf_instant_grid_update: NULL pointer");
  NERF_REQUIRE(((uintptr_t)workspace & 255) == 0, "nerf_instant_grid_update: workspace must be 256-byte aligned");
  if (hipMemsetAsync(active_count, 0, sizeof(unsigned long long), as_stream(stream)) != hipSuccess)
    return fail(NERF_ELAUNCH, "nerf_instant_grid_update: memset failed");
  for (int64_t c0 = 0; c0 < n_cells; c0 += slab_cells) {
    const int64_t n = n_cells - c0 < slab_cells ? n_cells - c0 : slab_cells;
    int rc;
    if (pts != nullptr) {
      rc = nerf_hash_encode_fwd_nat(pts + c0 * 3, n, table_f32, table_f16, n_levels, scale_host, res_host, size_host, offset_host, dense_host,
                                    hash_bound, workspace, 0, stream);
      if (rc != NERF_OK) return rc;
    } else {
      rc = hash_fwd_lattice(c0, n, resolution, grid_bound, table_f32, table_f16,
                            LevelArgs{n_levels, scale_host, res_host, size_host, offset_host, dense_host, hash_bound}, workspace, stream);
      if (rc != NERF_OK) return rc;
    }
    rc = imlp_sigma_grid(packed, workspace, n, grid + c0, binary_grid + c0, decay, dynamic, threshold, active_count, stream);
    if (rc != NERF_OK) return rc;
  }
  return NERF_OK;
}
