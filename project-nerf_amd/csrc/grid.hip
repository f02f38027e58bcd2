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
                            LevelArgs{n_levels, scale_host, res_host, size_host, offset_host, dense_host, hash_bound}, workspace, 0, stream);
      if (rc != NERF_OK) return rc;
    }
    rc = imlp_sigma_grid(packed, workspace, n, grid + c0, binary_grid + c0, decay, dynamic, threshold, active_count, stream);
    if (rc != NERF_OK) return rc;
  }
  return NERF_OK;
}

// ---- the Part 4 dual-hash field's refresh as one launch chain (reference DensityGrid.update in its dynamic form around
// NeuralField('part4'), src/renderer.py:62-86, 118-132, src/core.py:282-352) ----
// clear the count -> per slab of `slab_cells` cells, per time anchor k (t = 0, 0.5, 1): gather of deformation grid k ALONE at the
// lattice nodes (the triangle weights of an anchor are a unit vector) -> density-only deformation chain (x_c) -> canonical gather at
// x_c -> canonical sigma-net chain with the running maximum in its epilogue.  The first anchor of a slab folds against the decayed
// history, max(grid * decay, s0); the other two run with decay 1, so the cell ends as max(max(max(g d, s0), s1), s2) -- the
// reference's max(g d, max(s0, s1, s2)) (a maximum of non-NaN values does not depend on its grouping).  Only the last anchor's
// pass is given the count pointer (instant_sigma skips a NULL one): binary_grid and the count are those of the finished cell.
// The (slab, anchor) passes share ONE workspace; stream order serialises them.  12 * ceil(n_cells / slab_cells) + 1 enqueues.
namespace nerf {
struct P4GridWorkspace { size_t deform_nat, xc, canon_nat, total; };
static P4GridWorkspace p4_grid_workspace(int64_t slab_cells) {
  const size_t rows = ((size_t)slab_cells + 127) / 128 * 128;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  P4GridWorkspace w{};
  w.deform_nat = 0;
  w.xc = w.deform_nat + up(rows * 32 * 2);
  w.canon_nat = w.xc + up(rows * 3 * 4);
  w.total = w.canon_nat + up(rows * 32 * 2);
  return w;
}
}  // namespace nerf

extern "C" size_t nerf_p4_grid_update_workspace_bytes(int64_t slab_cells) {
  return slab_cells > 0 ? p4_grid_workspace(slab_cells).total : 0;
}

extern "C" int nerf_p4_grid_update(const void* packed, const float* params_f32, const float* const* tables_f32, const void* const* tables_f16,
                                   int deform_levels, const float* d_scale_host, const unsigned* d_res_host, const unsigned* d_size_host,
                                   const unsigned* d_offset_host, const unsigned* d_dense_host, int canon_levels, const float* c_scale_host,
                                   const unsigned* c_res_host, const unsigned* c_size_host, const unsigned* c_offset_host,
                                   const unsigned* c_dense_host, float hash_bound, int64_t n_cells, int resolution, float grid_bound,
                                   float* grid, uint8_t* binary_grid, float decay, float threshold, unsigned long long* active_count,
                                   int64_t slab_cells, void* workspace, nerf_stream_t stream) {
  NERF_REQUIRE((tables_f32 == nullptr) != (tables_f16 == nullptr),
               "nerf_p4_grid_update: exactly one of tables_f32 / tables_f16 (the four tables are all fp32 or all fp16)");
  for (int k = 0; k < 4; ++k)
    NERF_REQUIRE((tables_f32 != nullptr ? (const void*)tables_f32[k] : tables_f16[k]) != nullptr, "nerf_p4_grid_update: table %d is NULL", k);
  NERF_REQUIRE(deform_levels == 12 && canon_levels == 16,
               "nerf_p4_grid_update: deform_levels=%d, canon_levels=%d (the default-shape chains read 12 and 16 levels x 2 features)",
               deform_levels, canon_levels);
  NERF_REQUIRE(resolution >= 2 && resolution <= 32768, "nerf_p4_grid_update: resolution=%d (2..32768)", resolution);
  NERF_REQUIRE(n_cells == (int64_t)resolution * resolution * resolution, "nerf_p4_grid_update: n_cells=%lld is not resolution^3 (%d)",
               (long long)n_cells, resolution);
  NERF_REQUIRE(slab_cells > 0 && slab_cells % 128 == 0, "nerf_p4_grid_update: slab_cells=%lld (a positive multiple of 128)", (long long)slab_cells);
  NERF_REQUIRE(slab_cells * 32 < ((int64_t)1 << 31), "nerf_p4_grid_update: slab too large (slab_cells * 32 must stay below 2^31)");
  NERF_REQUIRE(workspace != nullptr, "nerf_p4_grid_update: workspace is NULL");
  NERF_REQUIRE(((uintptr_t)workspace & 255) == 0, "nerf_p4_grid_update: workspace must be 256-byte aligned");
  NERF_REQUIRE(hash_bound > 0.0f && grid_bound > 0.0f, "nerf_p4_grid_update: hash_bound and grid_bound must be positive");
  NERF_REQUIRE(packed && params_f32 && grid && binary_grid && active_count, "nerf_p4_grid_update: NULL pointer");
  NERF_REQUIRE(d_scale_host && d_res_host && d_size_host && d_offset_host && d_dense_host && c_scale_host && c_res_host && c_size_host &&
               c_offset_host && c_dense_host, "nerf_p4_grid_update: NULL level table");
  const LevelArgs lv_d{deform_levels, d_scale_host, d_res_host, d_size_host, d_offset_host, d_dense_host, hash_bound};
  const P4GridWorkspace w = p4_grid_workspace(slab_cells);
  char* ws = static_cast<char*>(workspace);
  float* xc = reinterpret_cast<float*>(ws + w.xc);
  if (hipMemsetAsync(active_count, 0, sizeof(unsigned long long), as_stream(stream)) != hipSuccess)
    return fail(NERF_ELAUNCH, "nerf_p4_grid_update: memset failed");
  const float anchors[3] = {0.0f, 0.5f, 1.0f};
  for (int64_t c0 = 0; c0 < n_cells; c0 += slab_cells) {
    const int64_t n = n_cells - c0 < slab_cells ? n_cells - c0 : slab_cells;
    for (int k = 0; k < 3; ++k) {
      int rc = hash_fwd_lattice(c0, n, resolution, grid_bound, tables_f32 ? tables_f32[k] : nullptr, tables_f16 ? tables_f16[k] : nullptr, lv_d,
                                ws + w.deform_nat, 1, stream);
      if (rc != NERF_OK) return rc;
      rc = p4_deform_lattice(packed, params_f32, ws + w.deform_nat, anchors[k], c0, n, resolution, grid_bound, xc, stream);
      if (rc != NERF_OK) return rc;
      rc = nerf_hash_encode_fwd_nat(xc, n, tables_f32 ? tables_f32[3] : nullptr, tables_f16 ? tables_f16[3] : nullptr, canon_levels, c_scale_host,
                                    c_res_host, c_size_host, c_offset_host, c_dense_host, hash_bound, ws + w.canon_nat, 1, stream);
      if (rc != NERF_OK) return rc;
      rc = p4_canon_sigma_grid(packed, ws + w.canon_nat, anchors[k], n, grid + c0, binary_grid + c0, k == 0 ? decay : 1.0f, threshold,
                               k == 2 ? active_count : nullptr, stream);
      if (rc != NERF_OK) return rc;
    }
  }
  return NERF_OK;
}

// ---- the Part 3 field's refresh (MLP deformation, hash-grid canonical field) as one launch chain (reference run.py:1191-1222: the
// union over 8-16 times through DensityGrid.update(..., decay=1.0), src/renderer.py:87-101, 118-132, around NeuralField('part3'),
// src/core.py:233-281, with the deformation MLP of src/decoders.py:165-195) ----
// clear the count -> per slab of `slab_cells` cells, per time j: deformation chain on the lattice nodes at the scalar time (x_c
// alone) -> canonical gather at x_c -> canonical sigma-net chain with the running maximum in its epilogue.  The first time of a slab
// folds against the decayed history, max(grid * decay, s_0); the others run with decay 1, so the cell ends as
// max(... max(max(g d, s_0), s_1) ..., s_{T-1}) -- with decay 1 the reference's sequence of updates.  Only the last time's pass is
// given the count pointer (instant_sigma skips a NULL one): binary_grid and the count are those of the finished cell.
// The (slab, time) passes share ONE workspace; stream order serialises them.  3 * n_times * ceil(n_cells / slab_cells) + 1 enqueues.
namespace nerf {
struct P3GridWorkspace { size_t xc, canon_nat, total; };
static P3GridWorkspace p3_grid_workspace(int64_t slab_cells) {
  const size_t rows = ((size_t)slab_cells + 127) / 128 * 128;
  auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  P3GridWorkspace w{};
  w.xc = 0;
  w.canon_nat = w.xc + up(rows * 3 * 4);
  w.total = w.canon_nat + up(rows * 32 * 2);
  return w;
}
}  // namespace nerf

extern "C" size_t nerf_p3_grid_update_workspace_bytes(int64_t slab_cells) {
  return slab_cells > 0 ? p3_grid_workspace(slab_cells).total : 0;
}

extern "C" int nerf_p3_grid_update(const void* packed_deform, const void* packed_canon, const float* table_f32, const void* table_f16,
                                   int canon_levels, const float* c_scale_host, const unsigned* c_res_host, const unsigned* c_size_host,
                                   const unsigned* c_offset_host, const unsigned* c_dense_host, float hash_bound, const float* times_host,
                                   int n_times, int64_t n_cells, int resolution, float grid_bound, float* grid, uint8_t* binary_grid,
                                   float decay, float threshold, unsigned long long* active_count, int64_t slab_cells, void* workspace,
                                   nerf_stream_t stream) {
  NERF_REQUIRE((table_f32 == nullptr) != (table_f16 == nullptr), "nerf_p3_grid_update: exactly one of table_f32 / table_f16");
  NERF_REQUIRE(canon_levels == 16, "nerf_p3_grid_update: canon_levels=%d (the default-shape sigma-net reads 16 levels x 2 features)", canon_levels);
  NERF_REQUIRE(n_times >= 1 && n_times <= 256, "nerf_p3_grid_update: n_times=%d (1..256)", n_times);
  NERF_REQUIRE(times_host != nullptr, "nerf_p3_grid_update: times_host is NULL");
  for (int j = 0; j < n_times; ++j)
    NERF_REQUIRE(__builtin_isfinite(times_host[j]), "nerf_p3_grid_update: times_host[%d] is not finite", j);
  NERF_REQUIRE(resolution >= 2 && resolution <= 32768, "nerf_p3_grid_update: resolution=%d (2..32768)", resolution);
  NERF_REQUIRE(n_cells == (int64_t)resolution * resolution * resolution, "nerf_p3_grid_update: n_cells=%lld is not resolution^3 (%d)",
               (long long)n_cells, resolution);
  NERF_REQUIRE(slab_cells > 0 && slab_cells % 128 == 0, "nerf_p3_grid_update: slab_cells=%lld (a positive multiple of 128)", (long long)slab_cells);
  NERF_REQUIRE(slab_cells * 32 < ((int64_t)1 << 31), "nerf_p3_grid_update: slab too large (slab_cells * 32 must stay below 2^31)");
  NERF_REQUIRE(workspace != nullptr, "nerf_p3_grid_update: workspace is NULL");
  NERF_REQUIRE(((uintptr_t)workspace & 255) == 0, "nerf_p3_grid_update: workspace must be 256-byte aligned");
  NERF_REQUIRE(hash_bound > 0.0f && grid_bound > 0.0f, "nerf_p3_grid_update: hash_bound and grid_bound must be positive");
  NERF_REQUIRE(packed_deform && packed_canon && grid && binary_grid && active_count, "nerf_p3_grid_update: NULL pointer");
  NERF_REQUIRE(c_scale_host && c_res_host && c_size_host && c_offset_host && c_dense_host, "nerf_p3_grid_update: NULL level table");
  const P3GridWorkspace w = p3_grid_workspace(slab_cells);
  char* ws = static_cast<char*>(workspace);
  float* xc = reinterpret_cast<float*>(ws + w.xc);
  if (hipMemsetAsync(active_count, 0, sizeof(unsigned long long), as_stream(stream)) != hipSuccess)
    return fail(NERF_ELAUNCH, "nerf_p3_grid_update: memset failed");
  for (int64_t c0 = 0; c0 < n_cells; c0 += slab_cells) {
    const int64_t n = n_cells - c0 < slab_cells ? n_cells - c0 : slab_cells;
    for (int j = 0; j < n_times; ++j) {
      int rc = p3_deform_lattice(packed_deform, times_host[j], c0, n, resolution, grid_bound, xc, stream);
      if (rc != NERF_OK) return rc;
      rc = nerf_hash_encode_fwd_nat(xc, n, table_f32, table_f16, canon_levels, c_scale_host, c_res_host, c_size_host, c_offset_host,
                                    c_dense_host, hash_bound, ws + w.canon_nat, 1, stream);
      if (rc != NERF_OK) return rc;
      rc = p4_canon_sigma_grid(packed_canon, ws + w.canon_nat, times_host[j], n, grid + c0, binary_grid + c0, j == 0 ? decay : 1.0f, threshold,
                               j == n_times - 1 ? active_count : nullptr, stream);
      if (rc != NERF_OK) return rc;
    }
  }
  return NERF_OK;
}
