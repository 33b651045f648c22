// Test-only device shim: the device twin of tests/host_math_shim.cpp.  The same gndt_math.hpp / gndt_cost.hpp /
// gndt_partition.hpp / gndt_bucket3.hpp functions the kernels inline, compiled by hipcc for gfx950 with libgndt's own flags
// (grid_ndt_amd/_lib.py: HIPCC_FLAGS) and run one thread per input, so the CPU tier's adversarial input families can be checked
// against the device build of that arithmetic (OCML's sqrtf / acosf / cosf, the fp64 divide and sqrt expansions, fmed3, fma).
// Every dshim_<name> takes the arguments of the host shim's shim_<name> (data pointers are device pointers here), then the stream;
// it returns hipGetLastError() of its launch.  Not part of the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gndt_bucket3.hpp"
#include "gndt_cost.hpp"
#include "gndt_math.hpp"

namespace {

constexpr int kThreads = 256;

inline dim3 grid_for(uint64_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

__device__ __forceinline__ uint64_t thread_index() { return (uint64_t)blockIdx.x * kThreads + threadIdx.x; }

struct Axes {
    float ox, oy, oz, gl, zl, ig, iz;
};

__global__ void __launch_bounds__(kThreads) k_point_keys(const float* xyz, uint64_t n, int stride, Axes A, int fast, uint64_t* keys,
                                                         uint8_t* ok) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    const float* p = xyz + i * stride;
    const gndt::PointKey k = fast ? gndt::point_key_fast(p[0], p[1], p[2], A.ox, A.oy, A.oz, A.gl, A.zl, A.ig, A.iz)
                                  : gndt::point_key(p[0], p[1], p[2], A.ox, A.oy, A.oz, A.gl, A.zl);
    keys[i] = gndt::pack_key(k.sx, k.sy, k.sz);
    ok[i] = k.ok;
}

// The bucket kernels' record -> (key, offset from the node's centre) sequence (k_bucket_direct, gndt_bucket3.hpp; k_bucket_blocked,
// gndt_blocked.hpp), restated here from the same three functions: axis_ceil_try on every axis, the IEEE divide on all three when
// any is undecided, then axis_index_offset per axis.  The kernels inline it; it is not a product function of its own.
__global__ void __launch_bounds__(kThreads) k_key_offset(const float* xyz, uint64_t n, int stride, Axes A, int32_t* s, double* v,
                                                         uint8_t* ok) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    const float* p = xyz + i * stride;
    const double hx = 0.5 * (double)A.gl, hz = 0.5 * (double)A.zl;
    bool und = false;
    float cx = gndt::axis_ceil_try(p[0], A.ox, A.ig, und);
    float cy = gndt::axis_ceil_try(p[1], A.oy, A.ig, und);
    float cz = gndt::axis_ceil_try(p[2], A.oz, A.iz, und);
    if (und) {
        cx = ceilf(fabsf(p[0] - A.ox) / A.gl);
        cy = ceilf(fabsf(p[1] - A.oy) / A.gl);
        cz = ceilf(fabsf(p[2] - A.oz) / A.zl);
    }
    bool good = true;
    int sx, sy, sz;
    double v0, v1, v2;
    gndt::axis_index_offset(p[0], A.ox, cx, (float)gndt::kMaxXY, hx, (double)A.ox, good, sx, v0);
    gndt::axis_index_offset(p[1], A.oy, cy, (float)gndt::kMaxXY, hx, (double)A.oy, good, sy, v1);
    gndt::axis_index_offset(p[2], A.oz, cz, (float)gndt::kMaxZ, hz, (double)A.oz, good, sz, v2);
    s[3 * i] = sx; s[3 * i + 1] = sy; s[3 * i + 2] = sz;
    v[3 * i] = v0; v[3 * i + 1] = v1; v[3 * i + 2] = v2;
    ok[i] = good;
}

__global__ void __launch_bounds__(kThreads) k_centres(const uint64_t* keys, uint64_t n, Axes A, double* c) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    int sx, sy, sz;
    gndt::unpack_key(keys[i], sx, sy, sz);
    c[3 * i] = gndt::axis_centre(sx, A.ox, A.gl);
    c[3 * i + 1] = gndt::axis_centre(sy, A.oy, A.gl);
    c[3 * i + 2] = gndt::axis_centre(sz, A.oz, A.zl);
}

__global__ void __launch_bounds__(kThreads) k_finalize(const uint32_t* count, const double* sums, const double* centres, uint64_t n,
                                                       int min_points, float* mean, float* cov, float* rough, float* normal) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    gndt::NodeResult r{};
    if ((int)count[i] >= min_points) gndt::finalize_node(count[i], sums + 9 * i, centres + 3 * i, r);
    for (int k = 0; k < 3; ++k) { mean[3 * i + k] = r.mean[k]; normal[3 * i + k] = r.normal[k]; }
    for (int k = 0; k < 6; ++k) cov[6 * i + k] = r.cov[k];
    rough[i] = r.rough;
}

__global__ void __launch_bounds__(kThreads) k_mean_z_n(const uint32_t* cnt, const double* sum_vz, const double* cz, uint64_t n, float* out) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    out[i] = gndt::node_mean_z(cnt[i], sum_vz[i], cz[i]);
}

__global__ void __launch_bounds__(kThreads) k_min_eigen(const double* S, uint64_t n, double* lam, double* vec) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    gndt::min_eigenpair_sym3(S + 6 * i, lam[i], vec + 3 * i);
}

__global__ void __launch_bounds__(kThreads) k_jacobi(const double* S, uint64_t n, double* evals, double* evecs) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    double ev[3], vv[3][3];
    gndt::eigen_sym3(S + 6 * i, ev, vv);
    for (int k = 0; k < 3; ++k) {
        evals[3 * i + k] = ev[k];
        for (int j = 0; j < 3; ++j) evecs[9 * i + 3 * k + j] = vv[k][j];
    }
}

__global__ void __launch_bounds__(kThreads) k_rough_normal(const double* S, uint64_t n, float* rough, float* normal) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    gndt::node_rough_normal(S + 6 * i, rough[i], normal + 3 * i);
}

__global__ void __launch_bounds__(kThreads) k_cost_angle(const float* n1, const float* n2, uint64_t n, float* out) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    out[i] = gndt::cost_angle(n1 + 3 * i, n2 + 3 * i);
}

__global__ void __launch_bounds__(kThreads) k_cost_travel(const float* cur, const float* des, uint64_t n, float* out) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    out[i] = gndt::cost_travel(cur + 3 * i, des + 3 * i);
}

// The integer helpers the build paths run on the device (the host runs them too): the key codec, the table hash, the column hash and its bucket (hashed,
// and through a block map when `blk` is on), the owner of a column among W ranks, the contiguous index.
struct IntOut {
    uint64_t* pack;      // pack_key(sx, sy, sz)
    int32_t* unpack;     // unpack_key of it, 3 per input
    uint64_t* mix;       // mix64(pack)
    uint32_t* chash;     // column_hash(sx, sy)
    uint32_t* bucket;    // column_bucket(sx, sy, P, B)
    uint32_t* owner;     // owner_of(sx, sy, W)
    int32_t* contig;     // contiguous_index(sx), contiguous_index(sy)
};

__global__ void __launch_bounds__(kThreads) k_ints(const int32_t* sx, const int32_t* sy, const int32_t* sz, uint64_t n,
                                                   gndt::GridParams P, uint32_t B, uint32_t W, IntOut o) {
    const uint64_t i = thread_index();
    if (i >= n) return;
    const uint64_t k = gndt::pack_key(sx[i], sy[i], sz[i]);
    o.pack[i] = k;
    int a, b, c;
    gndt::unpack_key(k, a, b, c);
    o.unpack[3 * i] = a; o.unpack[3 * i + 1] = b; o.unpack[3 * i + 2] = c;
    o.mix[i] = gndt::mix64(k);
    o.chash[i] = gndt::column_hash(sx[i], sy[i]);
    o.bucket[i] = gndt::column_bucket(sx[i], sy[i], P, B);
    o.owner[i] = gndt::owner_of(sx[i], sy[i], W);
    o.contig[2 * i] = gndt::contiguous_index(sx[i]);
    o.contig[2 * i + 1] = gndt::contiguous_index(sy[i]);
}

Axes axes(const float o[3], float gl, float zl) { return Axes{o[0], o[1], o[2], gl, zl, 1.0f / gl, 1.0f / zl}; }

// blk = {on, x0, y0, shx, shy, nx, ny}: the fields of BlockMap column_bucket reads
gndt::GridParams block_params(const int32_t blk[7]) {
    gndt::GridParams P{};
    P.blk.on = blk[0]; P.blk.x0 = blk[1]; P.blk.y0 = blk[2]; P.blk.shx = blk[3]; P.blk.shy = blk[4]; P.blk.nx = blk[5]; P.blk.ny = blk[6];
    return P;
}

}  // namespace

#define DSHIM_LAUNCH(kernel, n, stream, ...)                                                              \
    do {                                                                                                  \
        if ((n) > 0) hipLaunchKernelGGL(kernel, grid_for(n), dim3(kThreads), 0, stream, __VA_ARGS__);     \
        return (int)hipGetLastError();                                                                    \
    } while (0)

extern "C" {
int dshim_point_keys(const float* xyz, uint64_t n, int stride, const float o[3], float gl, float zl, uint64_t* keys, uint8_t* ok,
                     hipStream_t st) {
    DSHIM_LAUNCH(k_point_keys, n, st, xyz, n, stride, axes(o, gl, zl), 0, keys, ok);
}
int dshim_point_keys_fast(const float* xyz, uint64_t n, int stride, const float o[3], float gl, float zl, uint64_t* keys, uint8_t* ok,
                          hipStream_t st) {
    DSHIM_LAUNCH(k_point_keys, n, st, xyz, n, stride, axes(o, gl, zl), 1, keys, ok);
}
int dshim_key_offset(const float* xyz, uint64_t n, int stride, const float o[3], float gl, float zl, int32_t* s, double* v, uint8_t* ok,
                     hipStream_t st) {
    DSHIM_LAUNCH(k_key_offset, n, st, xyz, n, stride, axes(o, gl, zl), s, v, ok);
}
int dshim_centres(const uint64_t* keys, uint64_t n, const float o[3], float gl, float zl, double* c, hipStream_t st) {
    DSHIM_LAUNCH(k_centres, n, st, keys, n, axes(o, gl, zl), c);
}
int dshim_finalize(const uint32_t* count, const double* sums, const double* centres, uint64_t n, int min_points, float* mean, float* cov,
                   float* rough, float* normal, hipStream_t st) {
    DSHIM_LAUNCH(k_finalize, n, st, count, sums, centres, n, min_points, mean, cov, rough, normal);
}
int dshim_mean_z_n(const uint32_t* cnt, const double* sum_vz, const double* cz, uint64_t n, float* out, hipStream_t st) {
    DSHIM_LAUNCH(k_mean_z_n, n, st, cnt, sum_vz, cz, n, out);
}
int dshim_min_eigen(const double* S, uint64_t n, double* lam, double* vec, hipStream_t st) {
    DSHIM_LAUNCH(k_min_eigen, n, st, S, n, lam, vec);
}
int dshim_jacobi(const double* S, uint64_t n, double* evals, double* evecs, hipStream_t st) {
    DSHIM_LAUNCH(k_jacobi, n, st, S, n, evals, evecs);
}
int dshim_rough_normal(const double* S, uint64_t n, float* rough, float* normal, hipStream_t st) {
    DSHIM_LAUNCH(k_rough_normal, n, st, S, n, rough, normal);
}
int dshim_cost_angle(const float* n1, const float* n2, uint64_t n, float* out, hipStream_t st) {
    DSHIM_LAUNCH(k_cost_angle, n, st, n1, n2, n, out);
}
int dshim_cost_travel(const float* cur, const float* des, uint64_t n, float* out, hipStream_t st) {
    DSHIM_LAUNCH(k_cost_travel, n, st, cur, des, n, out);
}
int dshim_ints(const int32_t* sx, const int32_t* sy, const int32_t* sz, uint64_t n, const int32_t blk[7], uint32_t B, uint32_t W,
               uint64_t* pack, int32_t* unpack, uint64_t* mix, uint32_t* chash, uint32_t* bucket, uint32_t* owner, int32_t* contig,
               hipStream_t st) {
    DSHIM_LAUNCH(k_ints, n, st, sx, sy, sz, n, block_params(blk), B, W, IntOut{pack, unpack, mix, chash, bucket, owner, contig});
}
}
