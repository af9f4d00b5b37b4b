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

// ---- layouts more than one call takes (the element counts a kernel header fixes come in as arguments: no HIP here) ----
// hash_to_curve behind its first kernel: n rows of (u0, u1) in 48 Montgomery words, 2 n points of point_words words
struct H2cWork {
    Region<uint32_t> u, pts;
};
inline H2cWork h2c_work(Layout& L, size_t n, size_t point_words)
{
    H2cWork r;
    r.u = L.take<uint32_t>(48 * n);
    r.pts = L.take<uint32_t>(point_words * 2 * n);
    return r;
}

// The resident aggregate's verdicts over G groups (engine_resident_verify.cpp).  pe_verify_resident takes the front --
// head .. out, with the caller's point_of_row (por_bytes) and its message points (msg_bytes; 0: read in place).
// pe_verify_resident_data takes the same front with room for its own G message points and, behind it in the SAME buffer, what
// makes them: the tag, the groups' signing roots and hash_to_curve's work rows (dst_len > 0).
struct ResidentVerifyLayout {
    Region<uint8_t> head;          // -g1 in 256 bytes | point_of_row: one copy in
    Region<uint32_t> por;
    Region<uint8_t> msg;
    Region<uint32_t> off, ws;
    Region<int32_t> flag;
    Region<uint32_t> gt;
    Region<int32_t> gbad, fe;
    Region<uint32_t> ident;
    Region<int32_t> sub;
    Region<uint32_t> out, stats;   // counters | verdicts: one copy out
    Region<int32_t> verdict;
    Region<uint8_t> dst, roots;    // the data route only
    H2cWork h2c;
};
inline ResidentVerifyLayout resident_verify_layout(Layout& L, size_t G, size_t por_bytes, size_t msg_bytes, size_t pair_words,
                                                   size_t gt_words, size_t dst_len, size_t point_words)
{
    ResidentVerifyLayout r;
    r.head = L.take_bytes(256 + por_bytes);
    r.por = r.head.part<uint32_t>(256, por_bytes / 4);
    r.msg = L.take<uint8_t>(msg_bytes);
    r.off = L.take<uint32_t>(G + 1);
    r.ws = L.take<uint32_t>(pair_words * 2 * G);
    r.flag = L.take<int32_t>(2 * G);
    r.gt = L.take<uint32_t>(gt_words * G);
    r.gbad = L.take<int32_t>(G);
    r.fe = L.take<int32_t>(G);
    r.ident = L.take<uint32_t>(G);
    r.sub = L.take<int32_t>(G);
    r.out = L.take_bytes<uint32_t>(64 + 4 * G);
    r.stats = r.out.part<uint32_t>(0, 16);
    r.verdict = r.out.part<int32_t>(64, G);
    if (dst_len) {
        r.dst = L.take<uint8_t>(dst_len);
        r.roots = L.take<uint8_t>(32 * G);
        r.h2c = h2c_work(L, G, point_words);
    }
    return r;
}

}  // namespace posevo
