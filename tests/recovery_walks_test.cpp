// tests/recovery_walks_test.cpp -- TEST ONLY (test_recovery_walks_cpu.py).
//
// Scripted siamese.h call sequences around the decoder's recovery list and
// its readiness walk (DecoderCore::list_insert, check_recovery_possible),
// run against whichever implementation the first argument names (dlopen):
// the upstream reference to record the fixtures under tests/golden/walk_*.txt,
// the CPU test double (built with SGPU_WALK_CHECK, so every shortcut is
// compared with the full search / walk) to check against them.  Every call's
// result code and every recovered packet go to the event log on stdout.
//
//   recovery_walks_test <library.so | self> <sequence>
//
//   block       64 originals x 100 B in one block, 30 % of the originals and
//               of the recovery packets lost; is_ready (and decode when
//               ready) after every recovery packet
//   interleave  the same block, but a fifth of the received originals arrive
//               late, one between every two recovery packets (the got bits
//               change between packets of one key)
//   reorder     recovery packets of several windows held back and delivered
//               out of order: ends below and above the tail's run, equal ends
//               with another start (rows encoded after remove_before), and
//               duplicates
//   delete_run  a block short of packets completed by late originals (the
//               next expected packet passes the run: the list is emptied),
//               more packets of the same key, then a second block on the
//               same decoder
#include "../include/siamese.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

namespace {

struct Api
{
    int (*init)(int);
    SiameseEncoder (*enc_create)();
    void (*enc_free)(SiameseEncoder);
    SiameseResult (*enc_add)(SiameseEncoder, SiameseOriginalPacket*);
    SiameseResult (*enc_remove_before)(SiameseEncoder, unsigned);
    SiameseResult (*encode)(SiameseEncoder, SiameseRecoveryPacket*);
    SiameseDecoder (*dec_create)();
    void (*dec_free)(SiameseDecoder);
    SiameseResult (*dec_add_original)(SiameseDecoder, const SiameseOriginalPacket*);
    SiameseResult (*dec_add_recovery)(SiameseDecoder, const SiameseRecoveryPacket*);
    SiameseResult (*dec_is_ready)(SiameseDecoder);
    SiameseResult (*decode)(SiameseDecoder, SiameseOriginalPacket**, unsigned*);
};

template <class F> bool sym(void* h, const char* name, F& f)
{
    f = reinterpret_cast<F>(dlsym(h, name));
    if (!f)
        std::fprintf(stderr, "missing symbol %s\n", name);
    return f != nullptr;
}

// xorshift64*: the sequences are a function of the seed alone
struct Rng
{
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next()
    {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
    }
    bool pct(unsigned p) { return next() % 100 < p; }
};

uint64_t fnv(const uint8_t* p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) {
        h ^= p[i];
        h *= 1099511628211ull;
    }
    return h;
}

struct Run
{
    Api api;
    SiameseEncoder enc = nullptr;
    SiameseDecoder dec = nullptr;
    std::vector<std::vector<uint8_t>> sent;   // by packet number
    unsigned failures = 0;

    std::vector<uint8_t> payload(unsigned num, unsigned bytes)
    {
        std::vector<uint8_t> d(bytes);
        Rng r(1000003ull * num + bytes);
        for (uint8_t& b : d)
            b = (uint8_t)r.next();
        return d;
    }
    /// One more original into the encoder; returns its number
    unsigned send(unsigned bytes)
    {
        std::vector<uint8_t> d = payload((unsigned)sent.size(), bytes);
        SiameseOriginalPacket p;
        p.PacketNum = 0;
        p.DataBytes = bytes;
        p.Data = d.data();
        const SiameseResult r = api.enc_add(enc, &p);
        std::printf("enc_add %d %u\n", (int)r, p.PacketNum);
        if (r != Siamese_Success || p.PacketNum != sent.size())
            ++failures;
        sent.push_back(d);
        return p.PacketNum;
    }
    void deliver(unsigned num)
    {
        SiameseOriginalPacket p;
        p.PacketNum = num;
        p.DataBytes = (unsigned)sent[num].size();
        p.Data = sent[num].data();
        std::printf("add_orig %u %d\n", num, (int)api.dec_add_original(dec, &p));
    }
    std::vector<uint8_t> encode()
    {
        SiameseRecoveryPacket r;
        r.DataBytes = 0;
        r.Data = nullptr;
        const SiameseResult res = api.encode(enc, &r);
        std::vector<uint8_t> out;
        if (res == Siamese_Success)
            out.assign(r.Data, r.Data + r.DataBytes);
        std::printf("encode %d %u %016llx\n", (int)res, (unsigned)out.size(),
                    (unsigned long long)fnv(out.data(), out.size()));
        return out;
    }
    /// A recovery packet into the decoder, then is_ready and decodes while ready
    void recover(const std::vector<uint8_t>& rec)
    {
        SiameseRecoveryPacket r;
        r.DataBytes = (unsigned)rec.size();
        r.Data = rec.data();
        std::printf("add_rec %d\n", (int)api.dec_add_recovery(dec, &r));
        poll();
    }
    void poll()
    {
        for (int k = 0; k < 4; ++k) {
            const SiameseResult ready = api.dec_is_ready(dec);
            std::printf("ready %d\n", (int)ready);
            if (ready != Siamese_Success)
                break;
            SiameseOriginalPacket* out = nullptr;
            unsigned count = 0;
            const SiameseResult res = api.decode(dec, &out, &count);
            std::printf("decode %d %u\n", (int)res, count);
            if (res != Siamese_Success)
                continue;
            for (unsigned i = 0; i < count; ++i) {
                const SiameseOriginalPacket& p = out[i];
                std::printf("  got %u %u %016llx\n", p.PacketNum, p.DataBytes,
                            (unsigned long long)fnv(p.Data, p.DataBytes));
                if (p.PacketNum >= sent.size() || p.DataBytes != sent[p.PacketNum].size() ||
                    std::memcmp(p.Data, sent[p.PacketNum].data(), p.DataBytes) != 0) {
                    std::printf("  CORRUPT %u\n", p.PacketNum);
                    ++failures;
                }
            }
        }
    }
};

void seq_block(Run& t, bool interleave)
{
    Rng ch(interleave ? 77 : 42);
    const unsigned n = 64;
    for (unsigned i = 0; i < n; ++i)
        t.send(100);
    std::vector<unsigned> late;
    unsigned lost = 0;
    for (unsigned i = 0; i < n; ++i) {
        if (ch.pct(30))
            ++lost;
        else if (interleave && ch.pct(20))
            late.push_back(i);
        else
            t.deliver(i);
    }
    std::printf("lost %u late %u\n", lost, (unsigned)late.size());
    // (enough packets for the losses on both sides, then a few past ready)
    for (unsigned k = 0, kept = 0; k < 200 && kept < lost + (unsigned)late.size() + 6; ++k) {
        const std::vector<uint8_t> rec = t.encode();
        if (rec.empty() || ch.pct(30))
            continue;
        ++kept;
        t.recover(rec);
        if (interleave && kept % 2 == 0 && !late.empty()) {
            t.deliver(late.back());
            late.pop_back();
            t.poll();
        }
    }
}

void seq_reorder(Run& t)
{
    Rng ch(7);
    std::vector<std::vector<uint8_t>> held;
    unsigned next = 0;
    // windows growing by a few originals at a time; every row of a window
    // shares its end, rows after remove_before start later
    for (unsigned round = 0; round < 14; ++round) {
        const unsigned grow = 3 + ch.next() % 6;
        for (unsigned i = 0; i < grow; ++i) {
            const unsigned num = t.send(20 + ch.next() % 200);
            if (!ch.pct(30))
                t.deliver(num);
        }
        next += grow;
        const unsigned rows = 1 + ch.next() % 4;
        for (unsigned k = 0; k < rows; ++k) {
            if (k == 2 && next > 12) {
                const SiameseResult r = t.api.enc_remove_before(t.enc, next - 10);
                std::printf("remove_before %u %d\n", next - 10, (int)r);
            }
            const std::vector<uint8_t> rec = t.encode();
            if (!rec.empty())
                held.push_back(rec);
        }
        // every other round: what is held, in a shuffled order, one of them twice
        if (round % 2 == 1) {
            for (size_t i = held.size(); i > 1; --i)
                std::swap(held[i - 1], held[ch.next() % i]);
            for (size_t i = 0; i < held.size(); ++i) {
                t.recover(held[i]);
                if (i == 1)
                    t.recover(held[0]);
            }
            held.clear();
        }
    }
}

void seq_delete_run(Run& t)
{
    for (unsigned block = 0; block < 2; ++block) {
        const unsigned first = block * 40;
        for (unsigned i = 0; i < 40; ++i)
            t.send(60);
        std::vector<unsigned> late;
        for (unsigned i = 0; i < 40; ++i) {
            if (i % 8 == 1 || i % 8 == 6)
                late.push_back(first + i);   // (held back, not lost)
            else
                t.deliver(first + i);
        }
        std::vector<std::vector<uint8_t>> recs;
        for (unsigned k = 0; k < 9; ++k)
            recs.push_back(t.encode());
        // fewer packets than originals missing: the run grows, never ready
        for (unsigned k = 0; k < 4; ++k)
            t.recover(recs[k]);
        // the late originals: the last one moves the next expected packet
        // past the run's end, which empties the list
        // (the second block without asking: no decode takes them first)
        for (unsigned num : late) {
            t.deliver(num);
            if (block == 0)
                t.poll();
        }
        // the same key again (behind the window now), then on to the next block
        for (unsigned k = 4; k < 9; ++k)
            t.recover(recs[k]);
    }
}

} // namespace

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <library.so> block|interleave|reorder|delete_run\n", argv[0]);
        return 2;
    }
    // ("self": the implementation is linked into this program, the sanitizer build)
    void* h = dlopen(std::strcmp(argv[1], "self") ? argv[1] : nullptr, RTLD_NOW | RTLD_LOCAL);
    if (!h) {
        std::fprintf(stderr, "dlopen(%s): %s\n", argv[1], dlerror());
        return 2;
    }
    Run t;
    Api& a = t.api;
    if (!(sym(h, "siamese_init_", a.init) && sym(h, "siamese_encoder_create", a.enc_create) &&
          sym(h, "siamese_encoder_free", a.enc_free) && sym(h, "siamese_encoder_add", a.enc_add) &&
          sym(h, "siamese_encoder_remove_before", a.enc_remove_before) && sym(h, "siamese_encode", a.encode) &&
          sym(h, "siamese_decoder_create", a.dec_create) && sym(h, "siamese_decoder_free", a.dec_free) &&
          sym(h, "siamese_decoder_add_original", a.dec_add_original) &&
          sym(h, "siamese_decoder_add_recovery", a.dec_add_recovery) &&
          sym(h, "siamese_decoder_is_ready", a.dec_is_ready) && sym(h, "siamese_decode", a.decode)))
        return 2;
    if (a.init(SIAMESE_VERSION) != 0) {
        std::fprintf(stderr, "siamese_init failed\n");
        return 2;
    }
    t.enc = a.enc_create();
    t.dec = a.dec_create();
    const std::string name = argv[2];
    if (name == "block")
        seq_block(t, false);
    else if (name == "interleave")
        seq_block(t, true);
    else if (name == "reorder")
        seq_reorder(t);
    else if (name == "delete_run")
        seq_delete_run(t);
    else {
        std::fprintf(stderr, "unknown sequence %s\n", name.c_str());
        return 2;
    }
    a.enc_free(t.enc);
    a.dec_free(t.dec);
    std::printf("end failures %u\n", t.failures);
    return t.failures ? 1 : 0;
}
