// gndt_scratch.hpp — the carver: one scratch allocation cut into typed pieces by a bump pointer.  A consumer states its scratch ONCE, as
// a layout struct (next to its kernels) whose constructor takes the pieces off a Carver in order; run over a null base it gives the bytes
// to allocate (carve_scratch, gndt_handle.hpp), so no piece is carved without being counted.  No HIP: the CPU test tier builds it too.
#pragma once
#include <stdint.h>

namespace gndt {

#ifdef GNDT_SCRATCH_LOG             // the CPU test tier's build (tests/scratch_layout_shim.cpp): every piece noted as it is taken
struct ScratchPiece { uint64_t offset, elem, align, count; };
#endif

struct Carver {
    char* base;                     // null: take returns null and the carver only sizes
    uint64_t pos = 0;               // bytes taken so far: the allocation's size once the layout is through
    explicit Carver(void* b = nullptr) : base(static_cast<char*>(b)) {}
#ifdef GNDT_SCRATCH_LOG
    ScratchPiece* log = nullptr;    // room for the layout's pieces is the caller's
    uint32_t pieces = 0;
#endif

    // `count` elements of T at the next multiple of alignof(T).  Every layout runs from its widest alignment to its narrowest, so
    // nothing is padded; a piece of slack is taken like any other.
    template <typename T>
    T* take(uint64_t count) {
        pos = (pos + alignof(T) - 1) & ~(uint64_t)(alignof(T) - 1);
        T* p = base ? reinterpret_cast<T*>(base + pos) : nullptr;
#ifdef GNDT_SCRATCH_LOG
        if (log) log[pieces] = ScratchPiece{pos, sizeof(T), alignof(T), count};
        ++pieces;
#endif
        pos += count * sizeof(T);
        return p;
    }
};

}  // namespace gndt
