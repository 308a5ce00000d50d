// zr_direct_uv.hip — zr_direct.hip once more, as the build for scenes whose triangles carry texture coordinates (namespace zr::uvbuild)
#define ZR_UV 1
#include "zr_direct.hip"
