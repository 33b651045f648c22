// gndt_stream.hpp — load_once(): the load of records that no later kernel of the build reads again.
//
// The partition's intermediates each fit the chip's 256 MiB last-level cache on the bench scene, but a line stays there only until as
// many bytes again have been loaded or stored behind it: the stream a kernel reads for the LAST time pushes out what the same kernel is
// writing for the next one.  A non-temporal load (global_load_dwordx4 ... nt) does not displace resident lines, so the kernel's OUTPUT
// is what the next kernel finds (DESIGN §4.1 "Cache residency of the intermediates"; tools/ic_stream_probe.hip).
// The rule: only where one instruction takes whole lines; not for data a later kernel of the same build reads; not for stores.  It is
// a hint about caching, never about the value: records that are read once more after all (a bucket done again) are loaded correctly.
// Used by level 2 on recs1 and by k_bucket_blocked on recs; the sites measured and left plain are in profiles/r08_ablation.txt.
// -DGNDT_STREAM_NT=0 builds plain loads (an A/B through GNDT_EXTRA_CXXFLAGS, tools/ab_flags.sh).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef GNDT_STREAM_NT
#define GNDT_STREAM_NT 1
#endif

namespace gndt {

// a 16-byte record (the builtin takes the native vector type, not HIP's float4 struct)
__device__ __forceinline__ float4 load_once(const float4* p) {
#if GNDT_STREAM_NT
    typedef float native_f4 __attribute__((ext_vector_type(4)));
    const native_f4 v = __builtin_nontemporal_load(reinterpret_cast<const native_f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
#else
    return *p;
#endif
}

}  // namespace gndt
