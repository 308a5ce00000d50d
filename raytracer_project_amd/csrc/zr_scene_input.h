// zr_scene_input.h — the host half of a scene: the world as the caller gave it (SceneInput), and the error / environment helpers the host code reports
// through.  No HIP: zr_flatten.h builds on this header alone, so the flattener compiles and runs without the library (tests/native/flatten_check.cpp).
#pragma once
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/zr_capi.h"
#include "zr_bvh.h"
#include "zr_device_types.h"

namespace zr_host {
int fail(int code, const char* fmt, ...);          // sets the calling thread's zr_last_error() text, returns `code`
const char* last_error();
double env_double(const char* name, double dflt);  // a number from the environment (development switches), `dflt` when unset
const double kInf = std::numeric_limits<double>::infinity();
}
using zr_host::fail;
using zr_host::env_double;
using zr_host::kInf;

// one input array of a scene: the library's own copy (zr_scene_set_*) or a view of the caller's memory (zr_scene_set_all_borrowed)
template <class T>
struct HostArray {
    const T* p = nullptr; size_t n = 0;
    std::vector<T> own;
    void copy(const T* src, size_t count) { own.assign(src, src + count); p = own.data(); n = count; }
    void borrow(const T* src, size_t count) { std::vector<T>().swap(own); p = src; n = count; }
    void drop() { std::vector<T>().swap(own); p = nullptr; n = 0; }
    const T& operator[](size_t i) const { return p[i]; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    const T* data() const { return p; }
    T* own_data() { return own.empty() ? nullptr : own.data(); }   // the library's copy, writable (zr_scene_update_*); null for a view of the caller's memory
    const T* begin() const { return p; }
    const T* end() const { return p + n; }
};

// the world as given: copies, or borrowed views until the commit (zr_scene is this plus the device side)
struct SceneInput {
    HostArray<double> spheres, tri_v, tri_n, cubes;
    HostArray<double> tri_uv;       // per-vertex texture coordinates, 6 per triangle, or empty (zr_scene_set_triangle_uvs: always a copy)
    HostArray<uint32_t> sphere_mat, tri_mat, cube_mat;
    HostArray<zr_medium> media;
    HostArray<zr_xform_op> ops;
    HostArray<zr_object> objects;
    bool objects_set = false;
    std::vector<zr_group> groups;   // runs of triangles that ZR_PRIM_GROUP objects place (small: copied)
    std::vector<zr_material> materials;
    std::vector<zr_texture> textures;
    HostArray<unsigned char> texels;
};
