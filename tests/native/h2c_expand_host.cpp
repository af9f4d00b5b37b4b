// pos_evolution_amd/csrc/h2c_expand.h compiled for the HOST by a plain C++ compiler, from the very header k_h2c_expand includes:
// tests/test_hash_to_curve_model.py holds it to hashlib at the padding edges of the message and of the tag.
#include "../../pos_evolution_amd/csrc/h2c_expand.h"

using namespace posevo;

extern "C" {

// the 256 uniform bytes of expand_message_xmd(msg, dst, 256): b1 | ... | b8
void h2c_host_expand256(const uint8_t* msg, uint32_t msg_len, const uint8_t* dst, uint32_t dst_len, uint8_t* out256)
{
    H2cText t;
    t.msg = msg;
    t.dst = dst;
    t.msg_len = msg_len;
    t.dst_len = dst_len;
    uint32_t b0[8], prev[8] = {0, 0, 0, 0, 0, 0, 0, 0}, head[8];
    h2c_b0(b0, t);
    for (uint32_t idx = 1; idx <= 8; ++idx) {
        for (int j = 0; j < 8; ++j) head[j] = b0[j] ^ prev[j];
        h2c_bi(prev, head, idx, t);
        for (int j = 0; j < 8; ++j) {
            uint8_t* p = out256 + 32 * (idx - 1) + 4 * j;
            p[0] = (uint8_t)(prev[j] >> 24);
            p[1] = (uint8_t)(prev[j] >> 16);
            p[2] = (uint8_t)(prev[j] >> 8);
            p[3] = (uint8_t)prev[j];
        }
    }
}

}  // extern "C"
