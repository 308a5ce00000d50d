// zr_kernels_uv.hip — zr_kernels.hip once more, as the build for scenes whose triangles carry texture coordinates (namespace zr::uvbuild; see the top of
// zr_kernels.hip and DESIGN §14)
#define ZR_UV 1
#include "zr_kernels.hip"
