// uniform_slots_san.cpp -- stand-alone driver for a sanitizer build of the
// host control plane (uniform subwindows, encoder.h EncUniform).
//
// Linked with the library's host sources and the CPU test double of the
// backend (tools/backend_hostsim.cpp), all compiled with
// -fsanitize=address,undefined -DSGPU_SLOT_CHECK, into one program:
//
//   for f in siamese_amd/csrc/*.cpp tools/backend_hostsim.cpp tests/uniform_slots_san.cpp; do
//     g++ -std=c++17 -O1 -g -mavx2 -DSGPU_SLOT_CHECK -DSGPU_WALK_CHECK \
//         -fsanitize=address,undefined -fno-sanitize-recover=undefined -c $f -o $OUT/$(basename $f).o; done
//   g++ -fsanitize=address,undefined $OUT/*.o -o $OUT/uniform_slots_san -lpthread -ldl
//
// It drives encoder and decoder range adds over several subwindows, recovery
// rows from the descriptors (Cauchy and Siamese), a demotion by a differing
// length, one by a single add, a window restart, a decode of lost originals
// and the teardown of uniform, demoted and untouched subwindows.  Exit code 0
// and no sanitizer report is the pass criterion.
#include "../include/siamese_gpu.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                                                       \
    do {                                                                                                               \
        if (!(x)) {                                                                                                    \
            std::fprintf(stderr, "uniform_slots_san: %s failed (line %d)\n", #x, __LINE__);                           \
            return 1;                                                                                                  \
        }                                                                                                              \
    } while (0)

int main()
{
    CHECK(sgpu_init(-1) == 0);
    const unsigned kStride = 256, kCount = 200;
    std::vector<unsigned char> host((size_t)kStride * kCount);
    for (size_t i = 0; i < host.size(); ++i)
        host[i] = (unsigned char)((i * 131 + 7) % 251);
    unsigned char* dev = (unsigned char*)sgpu_device_alloc(host.size());
    CHECK(dev != nullptr);
    CHECK(sgpu_h2d(dev, host.data(), host.size()) == 0);

    for (unsigned variant = 0; variant < 4; ++variant) {
        SgpuEncoder enc = sgpu_encoder_create();
        SgpuDecoder dec = sgpu_decoder_create();
        CHECK(enc && dec);
        unsigned first = 0, added = 0;
        const unsigned n = variant == 0 ? 60 : 130;   // Cauchy rows / Siamese rows
        std::vector<unsigned> lens(n, 100);
        if (variant == 2)
            lens[70] = 90;   // demotes the second subwindow on a length
        CHECK(sgpu_encoder_add_range(enc, dev, kStride, lens.data(), 0, n, &first, &added) == Siamese_Success);
        CHECK(added == n && first == 0);
        if (variant == 3) {
            // a single add behind a range demotes the subwindow it lands in
            unsigned num = 0;
            CHECK(sgpu_encoder_add(enc, dev + (size_t)n * kStride, 100, &num) == Siamese_Success && num == n);
            lens.push_back(100);   // (never sent: one more for the decoder to recover)
        }
        // the decoder receives all but every fifth original, by ranges
        for (unsigned k = 0; k < n; k += 5) {
            unsigned calls = 0;
            const unsigned m = n - 1 - k < 4 ? n - 1 - k : 4;
            if (m == 0)
                break;
            CHECK(sgpu_decoder_add_original_range(dec, k + 1, dev + (size_t)(k + 1) * kStride, kStride, lens.data() + k + 1,
                                                  0, m, nullptr, &calls) == Siamese_Success);
            CHECK(calls == m);
        }
        const unsigned lost = (n + 4) / 5 + (variant == 3 ? 1 : 0);
        for (unsigned r = 0; r < lost + 2; ++r) {
            SgpuRecoveryPacket rec;
            CHECK(sgpu_encode(enc, &rec) == Siamese_Success);
            CHECK(sgpu_decoder_add_recovery(dec, &rec) == Siamese_Success);
            CHECK(sgpu_flush() == 0);
        }
        SiameseOriginalPacket* out = nullptr;
        unsigned count = 0;
        CHECK(sgpu_decode(dec, &out, &count) == Siamese_Success);
        CHECK(sgpu_flush() == 0);
        CHECK(count == lost);
        for (unsigned i = 0; i < count; ++i)
            CHECK(out[i].DataBytes == lens[out[i].PacketNum]);
        if (variant == 1) {
            // everything acknowledged, then a new range: the window restarts
            // and releases uniform subwindows, which are entered again
            CHECK(sgpu_encoder_remove_before(enc, n) == Siamese_Success);
            CHECK(sgpu_encoder_add_range(enc, dev, kStride, nullptr, 100, 70, &first, &added) == Siamese_Success);
            CHECK(added == 70 && first == n);
            SgpuRecoveryPacket rec;
            CHECK(sgpu_encode(enc, &rec) == Siamese_Success);
            CHECK(sgpu_flush() == 0);
        }
        sgpu_encoder_free(enc);
        sgpu_decoder_free(dec);
        CHECK(sgpu_flush() == 0);
    }
    sgpu_device_free(dev);
    std::printf("uniform_slots_san ok\n");
    return 0;
}
