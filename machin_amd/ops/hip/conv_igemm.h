// What the implicit-GEMM convolution sources share (conv_igemm.hip,
// conv_igemm_wrw.hip): the geometry table and the grid of persistent
// workgroups.
#pragma once
#include <cstdint>

// The geometry table: the two Nature layers. The lookup, the group
// sizes and the kernels' template arguments are all read from it.
struct cig_geom { int ksize, stride, cin, cout; };
#define CIG_NGEOM 2
static constexpr cig_geom CIG_GEOM[CIG_NGEOM] = {{4, 2, 32, 64},
                                                 {3, 1, 64, 64}};

// Index of the layer in the table, -1 for anything else.
int conv_igemm_geometry(int64_t cin, int64_t cout, int64_t ksize,
                        int64_t stride);

// 64 KB of LDS per workgroup: two resident workgroups per CU, and the
// grid is that many. MACHIN_CONV_IGEMM_WG overrides it (read per call);
// never more workgroups than groups of samples.
unsigned cig_grid(int64_t groups);
