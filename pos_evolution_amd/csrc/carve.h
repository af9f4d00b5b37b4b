// carve.h -- the layout of one synchronous call's scratch inside ONE growable device buffer.
//
//   Layout L;                                   1. offsets: every region taken, in order
//   const auto pk = L.take<uint8_t>(96 * n);
//   const auto status = L.take<int32_t>(n);
//   Workspace w;                                2. ONE ensure: bind (engine_internal.h) grows the buffer to L.total() ...
//   HIP_TRY(h, w.bind(h->d_batch, L, stream));
//   w.put(pk, pk96, 96 * n);                    3. ... and only then are there pointers: w(region), w.put / get / zero
//
// A region knows its element type and count: the byte count of a transfer is derived from them, and a transfer of more
// elements than the region holds is refused.  Pure offset arithmetic, no HIP: tests/test_carve_layout.py compiles this header
// with the host compiler alone.
#pragma once
#include <cassert>
#include <cstddef>
#include <cstdint>

namespace posevo {

constexpr size_t CARVE_ALIGN = 256;  // regions of one allocation start 256-byte aligned
inline size_t carve_up(size_t v) { return (v + CARVE_ALIGN - 1) & ~(CARVE_ALIGN - 1); }

template <typename T> struct Region {
    size_t off = 0, count = 0;  // byte offset from the buffer's base | elements of T
    size_t bytes() const { return count * sizeof(T); }
    bool holds(size_t n) const { return n <= count; }  // the bound every transfer checks: one comparison
    T* at(void* base) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + off); }
    // n elements of U, byte_off bytes into this region: the parts of a block that travels as ONE copy
    template <typename U> Region<U> part(size_t byte_off, size_t n) const
    {
        assert(byte_off % alignof(U) == 0 && byte_off + n * sizeof(U) <= bytes() && "carve: a part outside its region");
        return Region<U>{off + byte_off, n};
    }
};

struct Layout {
    size_t end = 0;  // bytes taken so far
    // `count` elements of T; the space is rounded up to the alignment, so a zero-count region takes none
    template <typename T> Region<T> take(size_t count)
    {
        const Region<T> r{carve_up(end), count};
        end = r.off + carve_up(r.bytes());
        return r;
    }
    // exactly `bytes` bytes, not rounded: the fixed-size heads, and a last block whose length is the length of its copy
    template <typename T = uint8_t> Region<T> take_bytes(size_t bytes)
    {
        const Region<T> r{carve_up(end), bytes / sizeof(T)};
        end = r.off + bytes;
        return r;
    }
    size_t total() const { return end; }
};

}  // namespace posevo
