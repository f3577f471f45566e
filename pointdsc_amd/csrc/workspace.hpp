// workspace.hpp -- the one bump allocator over a caller's workspace (host only;
// included by the launcher code of the translation units, by no device header).
//
// A stage writes its layout once, as a function of a Carve & and the shape that
// fills the stage's buffer struct.  The launcher runs it on the caller's
// pointer; the size query runs the same function on a null base and reads
// `off`, so a size and its layout cannot disagree.  A nested workspace passes
// the same Carve & down.
#pragma once
#include <cstddef>

namespace pdsc {

inline size_t align_bytes(size_t x) { return (x + 255) & ~size_t(255); }

struct Carve {
    char *base;      // null: a size query (every slice is null)
    size_t off = 0;  // the running size: every slice starts 256-byte aligned
    explicit Carve(void *p) : base(static_cast<char *>(p)) {}
    char *take_bytes(size_t n) {
        char *p = base ? base + off : nullptr;
        off += align_bytes(n);
        return p;
    }
    template <typename T> T *take(size_t n) { return reinterpret_cast<T *>(take_bytes(n * sizeof(T))); }
};

}  // namespace pdsc
