// engine_h2c.cpp -- hash_to_curve for G2 on the device: the message points H(m) every BLS call takes.
//   pe_hash_to_g2   n messages of one length -> n points: k_h2c_expand -> k_h2c_map -> k_h2c_finish
//   pe_map_to_g2    n x (u0, u1) -> n points: k_h2c_load_u -> k_h2c_map -> k_h2c_finish (the RFC's own seam: map_to_curve twice,
//                   the add, clear_cofactor)
// The suite is BLS12381G2_XMD:SHA-256_SSWU_RO_ (RFC 9380); tests/hash_to_curve_model.py is the specification.
// Both calls are synchronous on the engine's stream over a workspace in d_bls; one GPU: PE_ERR_STATE under pe_dist_init* and
// inside a pipeline.  The points may be written to device memory, where pe_verify_resident reads its message points.
#include "engine_internal.h"

using namespace posevo;

namespace {

// p, big-endian: a canonical word is below it
const uint8_t FP_P_BE48[48] = {
    0x1a, 0x01, 0x11, 0xea, 0x39, 0x7f, 0xe6, 0x9a, 0x4b, 0x1b, 0xa7, 0xb6, 0x43, 0x4b, 0xac, 0xd7,
    0x64, 0x77, 0x4b, 0x84, 0xf3, 0x85, 0x12, 0xbf, 0x67, 0x30, 0xd2, 0xa0, 0xf6, 0xb0, 0xf6, 0x24,
    0x1e, 0xab, 0xff, 0xfe, 0xb1, 0x53, 0xff, 0xff, 0xb9, 0xfe, 0xff, 0xff, 0xff, 0xff, 0xaa, 0xab};

constexpr uint32_t H2C_MAX_N = 1u << 24;  // 768 bytes of workspace a message

// what both calls share behind their own first kernel: (u0, u1) rows -> XYZZ points -> wire bytes
struct H2cTail {
    Region<uint32_t> u, pts;  // h2c_work (carve.h): pe_verify_resident_data takes the same two behind its own first kernel
    Region<uint8_t> out;
    Region<int32_t> st;
    bool out_in_place = false;
    MemKind out_kind = MemKind::Pageable;
};
H2cTail h2c_tail(Layout& L, uint32_t n, const uint8_t* out192, bool want_status)
{
    H2cTail t;
    t.out_kind = mem_kind(out192);
    t.out_in_place = reads_in_place(t.out_kind, out192);  // 16-byte aligned device memory: written where it lies
    const H2cWork work = h2c_work(L, n, H2C_POINT_WORDS);
    t.u = work.u;
    t.pts = work.pts;
    t.out = L.take<uint8_t>(t.out_in_place ? 0 : 192 * (size_t)n);
    t.st = L.take<int32_t>(want_status ? n : 0);
    return t;
}
int h2c_map_finish(pe_engine* h, const Workspace& w, const H2cTail& t, uint32_t n, uint8_t* out192, int32_t* status)
{
    hipStream_t s = h->stream;
    launch_h2c_map(s, w(t.u), 2 * n, w(t.pts));
    launch_h2c_finish(s, w(t.pts), n, t.out_in_place ? out192 : w(t.out), status ? w(t.st) : nullptr);
    HIP_TRY(h, hipGetLastError());
    if (!t.out_in_place)
        HIP_TRY(h, hipMemcpyAsync(out192, w(t.out), 192 * (size_t)n,
                                  t.out_kind == MemKind::Device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(h, w.get(t.st, status, n));
    HIP_TRY(h, hipStreamSynchronize(s));
    return PE_OK;
}
int h2c_enter(pe_engine* h, const char* who, uint32_t n)
{
    if (h->pipelining) return fail(h, PE_ERR_STATE, std::string(who) + ": inside a pipeline (the call is synchronous)");
    PE_TRY(enter(h));
    if (h->dist_ready()) return refuse_dist(h, who);
    if (n > H2C_MAX_N) return fail(h, PE_ERR_CAPACITY, std::string(who) + ": more than 2^24 messages in one call");
    return PE_OK;
}

}  // namespace

extern "C" {

int pe_hash_to_g2(pe_engine* h, const uint8_t* msgs, uint32_t n, uint32_t msg_len, const uint8_t* dst, uint32_t dst_len,
                  uint8_t* out192, int32_t* status)
{
    if (!h) return PE_ERR_INVALID_ARG;
    if (!dst || dst_len < 1 || dst_len > 255) return fail(h, PE_ERR_INVALID_ARG, "pe_hash_to_g2: the DST has 1 .. 255 bytes");
    if (msg_len > 255) return fail(h, PE_ERR_INVALID_ARG, "pe_hash_to_g2: messages of at most 255 bytes");
    if (n && (!out192 || (msg_len && !msgs))) return fail(h, PE_ERR_INVALID_ARG, "pe_hash_to_g2: no messages or no output");
    PE_TRY(h2c_enter(h, "pe_hash_to_g2", n));
    if (n == 0) return PE_OK;
    const size_t msg_bytes = (size_t)msg_len * n;
    const MemKind msg_kind = msg_bytes ? mem_kind(msgs) : MemKind::Pageable;
    const bool msg_in_place = msg_bytes == 0 || reads_in_place(msg_kind, msgs);
    Layout L;
    const auto r_dst = L.take<uint8_t>(dst_len);
    const auto r_msg = L.take<uint8_t>(msg_in_place ? 0 : msg_bytes);
    const H2cTail t = h2c_tail(L, n, out192, status != nullptr);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_bls, L, h->stream));
    HIP_TRY(h, w.put(r_dst, dst, dst_len));
    const uint8_t* d_msgs = nullptr;
    if (msg_bytes) HIP_TRY(h, device_view(w, r_msg, msg_kind, msgs, msg_bytes, &d_msgs));
    launch_h2c_expand(h->stream, d_msgs, n, msg_len, w(r_dst), dst_len, w(t.u));
    return h2c_map_finish(h, w, t, n, out192, status);
}

int pe_map_to_g2(pe_engine* h, const uint8_t* u_be, uint32_t n, uint8_t* out192)
{
    if (!h) return PE_ERR_INVALID_ARG;
    if (n && (!u_be || !out192)) return fail(h, PE_ERR_INVALID_ARG, "pe_map_to_g2: no input or no output");
    PE_TRY(h2c_enter(h, "pe_map_to_g2", n));
    if (n == 0) return PE_OK;
    for (size_t k = 0; k < 4 * (size_t)n; ++k)
        if (memcmp(u_be + 48 * k, FP_P_BE48, 48) >= 0)
            return fail(h, PE_ERR_INVALID_ARG, "pe_map_to_g2: a word of u is not below p");
    Layout L;
    const auto r_in = L.take<uint8_t>(192 * (size_t)n);
    const H2cTail t = h2c_tail(L, n, out192, false);
    Workspace w;
    HIP_TRY(h, w.bind(h->d_bls, L, h->stream));
    HIP_TRY(h, w.put(r_in, u_be, 192 * (size_t)n));
    launch_h2c_load_u(h->stream, w(r_in), 4 * n, w(t.u));
    return h2c_map_finish(h, w, t, n, out192, nullptr);
}

}  // extern "C"
