// tests/hostsim/backend_hostsim_deliver.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The hostsim backend's part for sgpu_decoder_deliver_range (linked into
// tests/hostsim/libsiamese_hostsim.so beside backend_hostsim.cpp, never into
// the product library): k_deliver in plain C++ (ops.h DeliverItem).  The
// prefix is read from the symbol (reference SiameseSerializers.h:598-640),
// checked against the symbol's readable bytes and the row, and the row gets
// the payload and a zero tail; an absent packet only its zero length word.
#include "../../siamese_amd/csrc/backend.h"

#include <cstdlib>
#include <cstring>

namespace sgpu {

namespace {

inline uint8_t* P(uint64_t a) { return reinterpret_cast<uint8_t*>(a); }

// header bytes (1..4) and *len, or -1 when `avail` bytes cannot hold the prefix
int deliver_prefix(const uint8_t* b, unsigned avail, unsigned* len)
{
    if (avail < 1)
        return -1;
    const unsigned top = b[0] >> 6;
    if (top <= 1) {
        *len = b[0];
        return 1;
    }
    if (top == 2) {
        if (avail < 2)
            return -1;
        *len = (((unsigned)b[0] << 8) | b[1]) & 0x3fff;
        return 2;
    }
    if ((b[0] & 0xE0) == 0xC0) {
        if (avail < 3)
            return -1;
        *len = (((unsigned)b[0] << 16) | ((unsigned)b[1] << 8) | b[2]) & 0x1fffff;
        return 3;
    }
    if (avail < 4)
        return -1;
    *len = (((unsigned)b[0] << 24) | ((unsigned)b[1] << 16) | ((unsigned)b[2] << 8) | b[3]) & 0x1fffffff;
    return 4;
}

} // namespace

void be_launch_deliver(const DeliverItem* items, uint32_t count, uint32_t)
{
    // (HOSTSIM_NOEXEC: the backend does no symbol work, backend_hostsim.cpp)
    static const bool noexec = std::getenv("HOSTSIM_NOEXEC") != nullptr;
    if (noexec)
        return;
    for (uint32_t i = 0; i < count; ++i) {
        const DeliverItem& it = items[i];
        const uint64_t stride = (uint64_t)it.stride16 << 4;
        unsigned h = 0, L = 0;
        if (it.src != 0 && it.cap != 0) {
            unsigned len = 0;
            const int hh = deliver_prefix(P(it.src), it.cap < 4 ? it.cap : 4, &len);
            if (hh >= 1 && len >= 1 && (unsigned)hh + len <= it.cap && len <= stride) {
                h = (unsigned)hh;
                L = len;
            }
        }
        const uint32_t lw = L;
        std::memcpy(P(it.lenOut), &lw, 4);
        if (it.src == 0)
            continue;
        for (uint64_t b = 0; b < stride; ++b)
            P(it.dst)[b] = b < L ? P(it.src)[h + b] : 0;
    }
}

} // namespace sgpu
