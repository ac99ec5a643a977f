// refseq_check.cpp -- TEST INFRASTRUCTURE: the three reference-preparation programs without a device.  Their own host code
// (rsem_amd/csrc/host/refprep_host.hpp and the three main()s) runs unchanged; the entry points it calls, rsem_refseq_*, are defined
// HERE and walk the same steps as rsem_amd/csrc/refseq.hip with the kernels' bodies of rsem_amd/csrc/refseq_block.hpp -- load_count,
// load_write and gather_span -- on tests/simt_emu.hpp (one OS thread per lane, "LDS" in memory): a wave a tile, a wave a span.
// Built with AddressSanitizer and UBSan (tests/test_refprep_cpu.py).  Never part of the product.
//
//   refseq_check extract <argv of rsem-extract-reference-transcripts>
//   refseq_check synthesis <argv of rsem-synthesis-reference-transcripts>
//   refseq_check preref <argv of rsem-preref>
//   refseq_check seams        the load and gather seam shapes of tests/test_refseq_gpu.py against plain loops
//   refseq_check limits       the byte values, degenerate records and segment counts of tests/refseq_limits.py against the same loops
// Build: hipcc (host compilation of the HIP headers simt_emu.hpp pulls in) -DRSEM_EMU -fsanitize=address,undefined -fno-gpu-sanitize
#include "simt_emu.hpp"

#include <functional>

#include "../rsem_amd/csrc/refseq_block.hpp"

#define main extract_main
#include "../rsem_amd/csrc/host/extract_reference.cpp"
#undef main
#define main synthesis_main
#include "../rsem_amd/csrc/host/synthesis_reference.cpp"
#undef main
#define main preref_main
#include "../rsem_amd/csrc/host/preref.cpp"
#undef main

using namespace rsem_refseqk;

struct rsem_refseq {
    std::vector<uint8_t> store;
    uint8_t* bases = nullptr;  // 16-byte aligned, kPad in front
    size_t bases_cap = 0;
    int64_t res_first = 0, res_n = 0;
    std::vector<uint64_t> res_base, res_bases;
    rsem_refseq_info info{};
    uint8_t* store_al = nullptr;
};

namespace {

std::string g_error;

// up to four waves at a time on one emulated workgroup: fn(wave index, lane)
void run_waves(uint64_t n_waves, const std::function<void(uint64_t, int)>& fn) {
    static emu::Block* blk = nullptr;
    if (!blk) {
        blk = new emu::Block();
        emu::barrier_init(&blk->bar, 256);
        for (int k = 0; k < 4; k++) emu::barrier_init(&blk->w[k].bar, 64);
    }
    for (uint64_t w0 = 0; w0 < n_waves; w0 += 4) {
        const int nw = (int)std::min<uint64_t>(4, n_waves - w0);
        std::vector<std::thread> th;
        for (int t = 0; t < nw * 64; t++)
            th.emplace_back([&, t]() { emu::t_tid = t; emu::t_blk = blk; fn(w0 + (uint64_t)(t >> 6), t & 63); });
        for (auto& t : th) t.join();
    }
}

uint8_t* aligned_bytes(size_t n) { return (uint8_t*)aligned_alloc(16, (n + 47) & ~(size_t)15); }

int fail(const char* msg) { g_error = msg; return RSEM_ERR_INVALID; }

}  // namespace

extern "C" const char* rsem_hip_strerror(int) { return "error"; }
extern "C" const char* rsem_hip_last_error(void) { return g_error.c_str(); }

extern "C" int rsem_refseq_create(rsem_refseq** out, int, uint64_t store_bytes) {
    rsem_refseq* h = new rsem_refseq();
    h->store_al = aligned_bytes((size_t)store_bytes);
    memset(h->store_al, '?', (size_t)store_bytes);
    h->store.resize((size_t)store_bytes);
    *out = h;
    return RSEM_OK;
}

extern "C" void rsem_refseq_destroy(rsem_refseq* h) {
    if (!h) return;
    free(h->store_al);
    free(h->bases);
    delete h;
}

extern "C" int rsem_refseq_load(rsem_refseq* h, int32_t mode, const uint8_t* raw, int64_t n_records, const uint64_t* body_lo, const uint64_t* body_hi,
                                const uint8_t* keep, int64_t first, int64_t* n_taken, uint64_t* n_bases, int64_t* bad) {
    uint64_t budget = 1ull << 20;
    if (const char* e = getenv("RSEM_REFSEQ_BATCH_BYTES")) {
        char* end = nullptr;
        const long long v = strtoll(e, &end, 10);
        if (end == e || *end || v < 1) return fail("RSEM_REFSEQ_BATCH_BYTES: a whole number from 1 on is expected");
        budget = (uint64_t)v;
    }
    const int64_t last = (int64_t)batch_end(body_lo, body_hi, (uint64_t)n_records, (uint64_t)first, budget);
    const uint32_t n = (uint32_t)(last - first);
    uint64_t kept_raw = 0;
    for (int64_t r = first; r < last; r++) {
        if (body_hi[r] < body_lo[r] || (r > first && body_lo[r] < body_hi[r - 1])) return fail("the bodies must ascend and lie apart");
        if (!keep || keep[r]) kept_raw += body_hi[r] - body_lo[r];
    }
    const uint64_t origin = body_lo[first] & ~15ull, raw_len = body_hi[last - 1] - origin, n_tiles = (raw_len + kTile - 1) / kTile;
    uint8_t* d_raw = aligned_bytes((size_t)raw_len);  // exactly what the device holds: nothing before the origin, 16 bytes' slack behind
    memset(d_raw, 0xee, (size_t)((raw_len + 47) & ~15ull));
    memcpy(d_raw, raw + origin, (size_t)raw_len);
    std::vector<uint64_t> lo(n), hi(n), bd(n, kNone), base(n, 0), end(n, 0), count(n_tiles + 1, 0), start(n_tiles + 1, 0);
    std::vector<uint8_t> kp(n);
    for (uint32_t i = 0; i < n; i++) { lo[i] = body_lo[first + i] - origin; hi[i] = body_hi[first + i] - origin; kp[i] = keep ? keep[first + i] != 0 : 1; }
    free(h->bases);
    h->bases = aligned_bytes((size_t)kept_raw + 2 * kPad);
    const Batch B{d_raw, raw_len, n, lo.data(), hi.data(), kp.data(), (uint32_t)mode};
    run_waves(n_tiles, [&](uint64_t t, int lane) { load_count(B, t, lane, count.data(), bd.data()); });
    for (uint64_t t = 0; t < n_tiles; t++) start[t + 1] = start[t] + count[t];
    if (start[n_tiles] > kept_raw) return fail("more bases than bytes");
    alignas(16) static uint8_t stage[4][kStage];
    run_waves(n_tiles, [&](uint64_t t, int lane) { load_write(B, t, lane, start.data(), h->bases + kPad, stage[t & 3], base.data(), end.data()); });
    free(d_raw);
    h->res_first = first;
    h->res_n = n;
    h->res_base.assign(n, 0);
    h->res_bases.assign(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (end[i] < base[i] || end[i] > start[n_tiles]) return fail("a record's bases lie outside the batch's");
        h->res_base[i] = base[i];
        h->res_bases[i] = n_bases[first + i] = end[i] - base[i];
        bad[first + i] = bd[i] == kNone ? -1 : (int64_t)(bd[i] + origin);
    }
    *n_taken = n;
    h->info.n_batches++;
    return RSEM_OK;
}

extern "C" int rsem_refseq_gather(rsem_refseq* h, int64_t n_segments, const int64_t* src, const uint32_t* first_base, const uint32_t* len, const uint64_t* dst,
                                  const uint32_t* flags) {
    const size_t n = (size_t)n_segments;
    if (!n) return RSEM_OK;
    std::vector<uint64_t> cum(n + 1, 0), sa(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (len[i] < 1 || dst[i] + len[i] > h->store.size()) return fail("a segment outside the store");
        if (i && dst[i] < dst[i - 1] + len[i - 1]) return fail("the destinations must ascend and lie apart");
        if (!(flags[i] & kFlagFill)) {
            const int64_t r = src[i] - h->res_first;
            if (r < 0 || r >= h->res_n || (uint64_t)first_base[i] + len[i] > h->res_bases[(size_t)r]) return fail("a segment outside its record");
            sa[i] = h->res_base[(size_t)r] + first_base[i];
        }
        cum[i + 1] = cum[i] + len[i];
    }
    if (!h->bases) h->bases = aligned_bytes(2 * kPad);
    const Segments S{(uint64_t)n, cum.data(), sa.data(), dst, flags};
    run_waves((cum[n] + kSpan - 1) / kSpan, [&](uint64_t w, int lane) { gather_span(S, w * kSpan, (w + 1) * kSpan, lane, h->bases + kPad, h->store_al); });
    return RSEM_OK;
}

extern "C" int rsem_refseq_download(rsem_refseq* h, uint64_t offset, uint64_t bytes, uint8_t* out) {
    if (offset + bytes > h->store.size()) return fail("outside the store");
    if (bytes) memcpy(out, h->store_al + offset, (size_t)bytes);
    return RSEM_OK;
}

extern "C" int rsem_refseq_get_info(rsem_refseq* h, rsem_refseq_info* info) { *info = h->info; return RSEM_OK; }

namespace {

// ---- the seam shapes against plain loops ---------------------------------------------------------------------------------

// the three maps spelled out here, from the reference's text, so that the kernels' own helpers are not what they are held to
bool plain_letter(uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }
uint8_t plain_check(uint8_t c) {  // extractRef.cpp:297-303
    switch (c) {
        case 'A': case 'C': case 'G': case 'T': case 'a': case 'c': case 'g': case 't': return c;
    }
    return c >= 'A' && c <= 'Z' ? 'N' : 'n';
}
uint8_t plain_flags(uint8_t c, uint32_t flags) {
    if (flags & 1u) {  // getOpp, utils.h:78-94
        switch (c) {
            case 'a': c = 't'; break; case 'c': c = 'g'; break; case 'g': c = 'c'; break; case 't': c = 'a'; break;
            case 'A': c = 'T'; break; case 'C': c = 'G'; break; case 'G': c = 'C'; break; case 'T': c = 'A'; break;
        }
    }
    if (flags & 2u) {  // RefSeqPolicy::convert
        if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 'a' + 'A');
        if (c != 'A' && c != 'C' && c != 'G' && c != 'T') c = 'N';
    }
    if ((flags & 4u) && c == 'N') c = 'G';  // AlignerRefSeqPolicy::convert
    return c;
}

int g_fail = 0;
void expect(bool ok, const char* what, long a = 0, long b = 0) {
    if (!ok) { fprintf(stderr, "refseq_check seams: %s (%ld, %ld)\n", what, a, b); g_fail++; }
}

// a file of records (header, body) and the plain result: bases per record (checked or raw), the first bad offset
void check_load(const std::string& file, int mode, const char* what) {
    const std::vector<rsemh::FastaRecord> recs = rsemh::frame_fasta(file.data(), file.size());
    const size_t n = recs.size();
    std::vector<uint64_t> lo(n), hi(n), nb(n);
    std::vector<int64_t> bad(n);
    std::vector<std::string> want(n);
    std::vector<int64_t> want_bad(n, -1);
    uint64_t total = 0;
    for (size_t r = 0; r < n; r++) {
        lo[r] = recs[r].lo; hi[r] = recs[r].hi;
        for (uint64_t p = lo[r]; p < hi[r]; p++) {
            const uint8_t c = (uint8_t)file[p];
            if (c == '\n') continue;
            if (mode == 1 && !plain_letter(c) && want_bad[r] < 0) want_bad[r] = (int64_t)p;
            want[r].push_back((char)(mode == 1 && plain_letter(c) ? plain_check(c) : c));
        }
        total += (want[r].size() + 15) & ~15ull;
    }
    rsem_refseq* h = nullptr;
    rsem_refseq_create(&h, 0, total);
    std::string got(total, '?');
    std::vector<uint64_t> place(n);
    for (int64_t first = 0; first < (int64_t)n;) {
        int64_t taken = 0;
        expect(rsem_refseq_load(h, mode, (const uint8_t*)file.data(), (int64_t)n, lo.data(), hi.data(), nullptr, first, &taken, nb.data(), bad.data()) == 0, what);
        std::vector<int64_t> src;
        std::vector<uint32_t> fb, ln, fl;
        std::vector<uint64_t> ds;
        uint64_t d = 0;
        for (int64_t r = 0; r < first + taken; r++) {
            if (r >= first && nb[r]) { src.push_back(r); fb.push_back(0); ln.push_back((uint32_t)nb[r]); fl.push_back(0); ds.push_back(d); }
            place[r] = d;
            d += (want[r].size() + 15) & ~15ull;
        }
        expect(rsem_refseq_gather(h, (int64_t)src.size(), src.data(), fb.data(), ln.data(), ds.data(), fl.data()) == 0, what);
        first += taken;
    }
    rsem_refseq_download(h, 0, total, (uint8_t*)&got[0]);
    for (size_t r = 0; r < n; r++) {
        expect(nb[r] == want[r].size(), what, (long)r, (long)nb[r]);
        expect(bad[r] == want_bad[r], what, (long)r, (long)bad[r]);
        if (mode == 0 || want_bad[r] < 0) expect(got.compare(place[r], want[r].size(), want[r]) == 0, what, (long)r, -1);
    }
    rsem_refseq_destroy(h);
}

std::string body_of(size_t raw_len, size_t width, uint32_t seed) {  // raw_len bytes of lines of `width` letters
    static const char* al = "ACGTacgtNnRyXk";
    std::string s;
    size_t col = 0;
    while (s.size() < raw_len) {
        if (col == width) { s.push_back('\n'); col = 0; continue; }
        seed = seed * 1664525u + 1013904223u;
        s.push_back(al[(seed >> 24) % 14]);
        col++;
    }
    return s;
}

int seams() {
    const size_t T = kTile, C = kChunk;
    for (int mode = 0; mode < 2; mode++) {
        for (size_t len : {(size_t)1, (size_t)15, (size_t)16, (size_t)17, C - 1, C, C + 1, T - 1, T, T + 1, 2 * T + 3})
            for (size_t width : {(size_t)60, (size_t)1})
                check_load(">a\n" + body_of(len, width, (uint32_t)len) + "\n>b x\n" + body_of(33, 7, 5), mode, "load lengths");
        // a line end as the last and as the first byte of a tile; no final line end; empty lines over a tile's edge; two tiny records in one chunk
        std::string s = ">a\n" + body_of(T - 4, 1000000, 1) + "\n" + body_of(50, 60, 2);
        check_load(s, mode, "line end last in tile");
        s = ">a\n" + body_of(T - 3, 1000000, 1) + "\n" + body_of(50, 60, 2);
        check_load(s, mode, "line end first in tile");
        s = ">a\n" + body_of(T - 10, 1000000, 3) + std::string(20, '\n') + "ACGT\n";
        check_load(s, mode, "empty lines over the edge");
        check_load(">a\nAC\n>b\nG\n>c\nT", mode, "tiny records");
        s = ">a\n" + body_of(T - 3, 1000000, 4);
        s[T - 1] = '*';
        s += "\n>b\n" + body_of(2 * T, 60, 5);
        s[s.size() - 1 - T] = '-';
        s[s.size() - 7] = '*';
        check_load(s, mode, "bad bytes");
        s = ">a*\nACGT\n>b *\nAC";
        check_load(s, mode, "bad byte in a header");
        s = ">a\n" + body_of(T, 1000000, 6);
        s[T] = '.';
        check_load(s, mode, "bad byte first in tile");
    }
    // gather: every misalignment, the spans' seams, the flags
    const std::string chr = body_of(3 * kSpan + 100, 1000000, 9);
    const std::string file = ">c\n" + chr + "\n";
    std::vector<uint64_t> lo{3}, hi{3 + chr.size()}, nb(1);
    std::vector<int64_t> bad(1);
    auto plain = [&](uint32_t first, uint32_t len, uint32_t flags) {
        std::string o;
        for (uint32_t p = 0; p < len; p++)
            o.push_back((flags & kFlagFill) ? 'A' : (char)plain_flags((uint8_t)chr[(flags & kFlagRC) ? first + len - 1 - p : first + p], flags));
        return o;
    };
    auto run = [&](const std::vector<uint32_t>& fb, const std::vector<uint32_t>& ln, const std::vector<uint64_t>& ds, const std::vector<uint32_t>& fl, const char* what) {
        const uint64_t total = ds.back() + ln.back() + 40;
        rsem_refseq* h = nullptr;
        rsem_refseq_create(&h, 0, total);
        int64_t taken = 0;
        rsem_refseq_load(h, 0, (const uint8_t*)file.data(), 1, lo.data(), hi.data(), nullptr, 0, &taken, nb.data(), bad.data());
        std::vector<int64_t> src(fb.size(), 0);
        expect(rsem_refseq_gather(h, (int64_t)fb.size(), src.data(), fb.data(), ln.data(), ds.data(), fl.data()) == 0, what);
        std::string got(total, ' '), want(total, '?');
        rsem_refseq_download(h, 0, total, (uint8_t*)&got[0]);
        for (size_t i = 0; i < fb.size(); i++) want.replace(ds[i], ln[i], plain(fb[i], ln[i], fl[i]));
        expect(got == want, what);
        rsem_refseq_destroy(h);
    };
    for (uint32_t flags : {0u, 1u, 2u, 3u, 6u, 7u}) {
        std::vector<uint32_t> fb, ln, fl;
        std::vector<uint64_t> ds;
        uint64_t d = 0;
        for (uint32_t sm = 0; sm < 16; sm++)
            for (uint32_t dm = 0; dm < 16; dm++)
                for (uint32_t len : {1u, 15u, 16u, 17u, 50u}) {
                    d = ((d + 15) & ~15ull) + dm;
                    fb.push_back(16 + sm); ln.push_back(len); ds.push_back(d); fl.push_back(flags);
                    d += len;
                }
        run(fb, ln, ds, fl, "misalignments");
    }
    for (uint32_t e : {kSpan - 1, kSpan, kSpan + 1, 3 * kSpan + 50})
        for (uint32_t flags : {0u, 1u}) run({5, 1, 0}, {e, 7, 3}, {3, e + 20, e + 40}, {flags, flags, kFlagFill}, "span seams");
    return g_fail ? 1 : 0;
}

// ---- the limit shapes of tests/refseq_limits.py against the same plain loops ------------------------------------------------------

struct Seg { int64_t src; uint32_t first, len; uint64_t dst; uint32_t flags; };

void set_budget(uint64_t b) {  // 0: unset
    if (b) setenv("RSEM_REFSEQ_BATCH_BYTES", std::to_string(b).c_str(), 1); else unsetenv("RSEM_REFSEQ_BATCH_BYTES");
}

std::string any_letters(size_t n, size_t width, uint32_t seed) {  // A-Z and a-z, a line end after every `width` of them (0: none)
    std::string s;
    size_t col = 0;
    while (s.size() < n) {
        if (width && col == width) { s.push_back('\n'); col = 0; continue; }
        seed = seed * 1664525u + 1013904223u;
        const uint32_t k = (seed >> 16) % 52;
        s.push_back((char)(k < 26 ? 'A' + k : 'a' + (k - 26)));
        col++;
    }
    return s;
}

uint64_t batches_of(const std::vector<uint64_t>& lo, const std::vector<uint64_t>& hi, uint64_t budget) {
    uint64_t n = 0;
    for (uint64_t first = 0; first < lo.size(); n++) first = batch_end(lo.data(), hi.data(), lo.size(), first, budget);
    return n;
}

// check_load on records given as arrays: every record that has bases (in checked mode: and no bad byte) is copied to a place of its own,
// at an odd offset of a store that a fill segment has covered before; n_bases, bad, the whole store and the number of batches
void check_load_arrays(const std::string& raw, const std::vector<uint64_t>& lo, const std::vector<uint64_t>& hi, const std::vector<uint8_t>* keep, int mode, uint64_t budget,
                       const char* what) {
    set_budget(budget);
    const size_t n = lo.size();
    std::vector<std::string> want(n);
    std::vector<int64_t> want_bad(n, -1), bad(n, -7);
    std::vector<uint64_t> nb(n, 77), place(n);
    uint64_t total = 1;
    for (size_t r = 0; r < n; r++) {
        for (uint64_t p = lo[r]; p < hi[r]; p++) {
            const uint8_t c = (uint8_t)raw[p];
            if (c == '\n') continue;
            if (mode == 1 && !plain_letter(c) && want_bad[r] < 0) want_bad[r] = (int64_t)p;
            if (!keep || (*keep)[r]) want[r].push_back((char)(mode == 1 && plain_letter(c) ? plain_check(c) : c));
        }
        place[r] = total;
        total += ((want[r].size() + 15) & ~15ull) + 16;
    }
    total += 16;
    rsem_refseq* h = nullptr;
    rsem_refseq_create(&h, 0, total);
    {
        const int64_t src = 0;
        const uint32_t fb = 0, ln = (uint32_t)total, fl = kFlagFill;
        const uint64_t ds = 0;
        expect(rsem_refseq_gather(h, 1, &src, &fb, &ln, &ds, &fl) == 0, what);
    }
    std::string expected(total, 'A'), got(total, '?');
    for (int64_t first = 0; first < (int64_t)n;) {
        int64_t taken = 0;
        expect(rsem_refseq_load(h, mode, (const uint8_t*)raw.data(), (int64_t)n, lo.data(), hi.data(), keep ? keep->data() : nullptr, first, &taken, nb.data(), bad.data()) == 0, what);
        if (taken < 1) { expect(false, "nothing taken"); break; }
        std::vector<int64_t> src;
        std::vector<uint32_t> fb, ln, fl;
        std::vector<uint64_t> ds;
        for (int64_t r = first; r < first + taken; r++)
            if (nb[r] && bad[r] < 0) { src.push_back(r); fb.push_back(0); ln.push_back((uint32_t)nb[r]); fl.push_back(0); ds.push_back(place[r]); }
        expect(rsem_refseq_gather(h, (int64_t)src.size(), src.data(), fb.data(), ln.data(), ds.data(), fl.data()) == 0, what);
        first += taken;
    }
    rsem_refseq_download(h, 0, total, (uint8_t*)&got[0]);
    for (size_t r = 0; r < n; r++) {
        expect(nb[r] == want[r].size(), what, (long)r, (long)nb[r]);
        expect(bad[r] == want_bad[r], what, (long)r, (long)bad[r]);
        if (mode == 0 || want_bad[r] < 0) expected.replace(place[r], want[r].size(), want[r]);
    }
    expect(got == expected, what, -1, -1);
    expect((uint64_t)h->info.n_batches == (budget ? batches_of(lo, hi, budget) : 1), what, -2, h->info.n_batches);
    rsem_refseq_destroy(h);
}

// the records loaded batch after batch (raw mode), each batch followed by the segments that read from it; the fill of the whole store first
void check_gather_arrays(const std::string& raw, const std::vector<uint64_t>& lo, const std::vector<uint64_t>& hi, const std::vector<Seg>& segs, uint64_t size, uint64_t budget,
                         const char* what) {
    set_budget(budget);
    const size_t n = lo.size();
    std::vector<std::string> bases(n);
    for (size_t r = 0; r < n; r++)
        for (uint64_t p = lo[r]; p < hi[r]; p++)
            if (raw[p] != '\n') bases[r].push_back(raw[p]);
    std::string want(size, 'A'), got(size, '?');
    for (const Seg& s : segs)
        for (uint32_t p = 0; p < s.len; p++)
            want[s.dst + p] = (s.flags & kFlagFill) ? 'A' : (char)plain_flags((uint8_t)bases[(size_t)s.src][(s.flags & kFlagRC) ? s.first + s.len - 1 - p : s.first + p], s.flags);
    rsem_refseq* h = nullptr;
    rsem_refseq_create(&h, 0, size);
    {
        const int64_t src = 0;
        const uint32_t fb = 0, ln = (uint32_t)size, fl = kFlagFill;
        const uint64_t ds = 0;
        expect(rsem_refseq_gather(h, 1, &src, &fb, &ln, &ds, &fl) == 0, what);
    }
    std::vector<uint64_t> nb(n);
    std::vector<int64_t> bad(n);
    for (int64_t first = 0; first < (int64_t)n;) {
        int64_t taken = 0;
        expect(rsem_refseq_load(h, 0, (const uint8_t*)raw.data(), (int64_t)n, lo.data(), hi.data(), nullptr, first, &taken, nb.data(), bad.data()) == 0, what);
        if (taken < 1) { expect(false, "nothing taken"); break; }
        std::vector<int64_t> src;
        std::vector<uint32_t> fb, ln, fl;
        std::vector<uint64_t> ds;
        for (const Seg& s : segs)
            if (s.src >= first && s.src < first + taken) { src.push_back(s.src); fb.push_back(s.first); ln.push_back(s.len); fl.push_back(s.flags); ds.push_back(s.dst); }
        expect(rsem_refseq_gather(h, (int64_t)src.size(), src.data(), fb.data(), ln.data(), ds.data(), fl.data()) == 0, what);
        first += taken;
    }
    rsem_refseq_download(h, 0, size, (uint8_t*)&got[0]);
    for (size_t r = 0; r < n; r++) expect(nb[r] == bases[r].size(), what, (long)r, (long)nb[r]);
    expect(got == want, what, -1, -1);
    rsem_refseq_destroy(h);
}

int limits() {
    const uint64_t T = kTile, C = kChunk;
    // every byte value, raw mode: one record, the 255 values three times; flag sets 0..7 from an odd source offset to odd destinations
    {
        std::string body;
        for (int rep = 0; rep < 3; rep++)
            for (int v = 0; v < 256; v++)
                if (v != '\n') body.push_back((char)v);
        const std::string raw = ">raw\n" + body + "\n";
        const std::vector<uint64_t> lo{5}, hi{5 + body.size()};
        std::vector<Seg> segs;
        uint64_t d = 3;
        for (uint32_t f = 0; f < 8; f++) { segs.push_back(Seg{0, 1, (uint32_t)body.size() - 2, d, f}); d += body.size() + 5; }
        for (uint64_t budget : {(uint64_t)0, (uint64_t)1}) {
            check_load_arrays(raw, lo, hi, nullptr, 0, budget, "every byte, raw");
            check_gather_arrays(raw, lo, hi, segs, d + 11, budget, "every byte, the flag sets");
        }
    }
    // every byte value, checked mode: 255 records AC?GT, seven bytes apart
    {
        std::string raw;
        std::vector<uint64_t> lo, hi;
        for (int v = 0; v < 256; v++) {
            if (v == '\n') continue;
            raw += ">\n";
            lo.push_back(raw.size());
            raw += "AC";
            raw.push_back((char)v);
            raw += "GT";
            hi.push_back(raw.size());
        }
        for (uint64_t budget : {(uint64_t)0, (uint64_t)40}) check_load_arrays(raw, lo, hi, nullptr, 1, budget, "every byte, checked");  // (40: six records a batch)
    }
    // empty and adjacent bodies
    {
        const uint64_t size = 2 * T + 819;
        std::string raw = any_letters(size, 61, 17);
        for (uint64_t p = 3060; p < 3090; p++) raw[p] = '\n';
        raw[2105] = '*';
        raw[2150] = '-';
        const std::vector<uint64_t> lo{0, 0, 16, 16, 40, 48, 48, 50, C, C, 1030, 2 * C, 2100, 2112, 2200, 3060, 3090, T, T, 4200, 2 * T, 8253, 8260, 8300, 9000, size};
        const std::vector<uint64_t> hi{0, 16, 16, 40, 40, 48, 48, C, C, 1030, 2 * C, 2100, 2112, 2200, 3060, 3090, T, T, 4200, 2 * T, 8250, 8253, 8300, 9000, size, size};
        std::vector<uint8_t> alt(lo.size());
        for (size_t r = 0; r < alt.size(); r++) alt[r] = (uint8_t)(1 - r % 2);
        for (int mode = 0; mode < 2; mode++)
            for (uint64_t budget : {(uint64_t)0, (uint64_t)6, (uint64_t)1}) {  // (6: the smallest body that has a byte, 1024..1030)
                if (budget == 6 && mode == 0) continue;
                check_load_arrays(raw, lo, hi, nullptr, mode, budget, "empty and adjacent bodies");
                check_load_arrays(raw, lo, hi, &alt, mode, budget, "empty and adjacent bodies, keep alternating");
            }
        // a call whose only record is empty: no byte uploaded at a multiple of 16
        const std::vector<uint8_t> none{0};
        for (uint64_t off : {(uint64_t)32, (uint64_t)21})
            for (int mode = 0; mode < 2; mode++)
                for (uint64_t budget : {(uint64_t)0, (uint64_t)1}) {
                    check_load_arrays(raw.substr(0, 64), {off}, {off}, nullptr, mode, budget, "a lone empty record");
                    check_load_arrays(raw.substr(0, 64), {off}, {off}, &none, mode, budget, "a lone empty record, not kept");
                }
    }
    // 256 bodies of one byte, a byte apart: eight records to a lane
    for (int variant = 0; variant < 3; variant++) {
        std::string raw = ">dense....\n" + std::string(53, '\n');
        std::vector<uint64_t> lo, hi;
        const std::string bodies = any_letters(256, 0, 5 + (uint32_t)variant);
        for (int k = 0; k < 256; k++) {
            lo.push_back(raw.size());
            raw.push_back(variant == 2 && k % 7 == 3 ? "*-[`{@~"[k / 7 % 7] : bodies[(size_t)k]);
            hi.push_back(raw.size());
            raw.push_back(variant == 1 && k % 4 == 0 ? "*\x01\x80\xff"[k / 4 % 4] : '\n');
        }
        std::vector<uint8_t> alt(256);
        for (size_t r = 0; r < 256; r++) alt[r] = (uint8_t)(r % 2);
        for (int mode = 0; mode < 2; mode++) {
            check_load_arrays(raw, lo, hi, &alt, mode, 0, "dense records, keep alternating");
            check_load_arrays(raw, lo, hi, nullptr, mode, 0, "dense records");
        }
        if (variant == 2) {  // (a launch is 64 OS threads here: a batch each for the first 64 records only)
            const std::vector<uint64_t> lo64(lo.begin(), lo.begin() + 64), hi64(hi.begin(), hi.begin() + 64);
            check_load_arrays(raw, lo64, hi64, &alt, 1, 1, "dense records, a batch each");
        }
    }
    // gather: the segment counts, the two ends of the bases, the two ends of the store
    {
        const std::string s0 = any_letters(kGroupSpan + 20, 0, 29), s1 = any_letters(333, 0, 31);
        std::string raw = ">c0\n";
        std::vector<uint64_t> lo, hi;
        for (const std::string* s : {&s0, &s1}) {
            if (s == &s1) raw += "\n>c1\n";
            lo.push_back(raw.size());
            for (size_t i = 0; i < s->size(); i += 70) { if (i) raw.push_back('\n'); raw += s->substr(i, 70); }
            hi.push_back(raw.size());
        }
        raw.push_back('\n');
        for (uint64_t budget : {(uint64_t)0, (uint64_t)1}) {
            std::vector<Seg> segs;
            for (uint32_t i = 0; i < 5000; i++) segs.push_back(Seg{0, (7 * i) % 16000, 1, 2 + 3ull * i, i % 8});
            check_gather_arrays(raw, lo, hi, segs, 3 * 5000 + 8, budget, "5000 segments of one base");
            for (uint32_t len : {kSpan, kGroupSpan}) {
                segs.clear();
                uint64_t d = 5;
                uint32_t k = 0;
                for (uint32_t flags : {0u, 1u, 7u}) { segs.push_back(Seg{0, k++, len, d, flags}); d += len + 9; }
                check_gather_arrays(raw, lo, hi, segs, d + 16, budget, "spans that are one segment");
            }
            segs.clear();
            uint64_t d = 0;
            for (uint32_t flags : {0u, 1u, 3u})
                for (uint32_t dm = 0; dm < 16; dm++)
                    for (uint32_t len : {1u, 15u, 16u, 17u, 40u}) {
                        d = ((d + 15) & ~15ull) + dm;
                        segs.push_back(Seg{0, 0, len, d, flags});
                        d += len;
                        d = ((d + 15) & ~15ull) + dm;
                        segs.push_back(Seg{1, (uint32_t)s1.size() - len, len, d, flags});
                        d += len;
                    }
            check_gather_arrays(raw, lo, hi, segs, d + 20, budget, "the two ends of the bases");
        }
        for (uint32_t len : {1u, 17u, 40u})
            for (uint32_t flags : {0u, 1u})
                check_gather_arrays(raw, lo, hi, {Seg{1, 3, len, 0, flags}, Seg{1, 50, len, 203 - len, flags}}, 203, 0, "the two ends of the store");
    }
    return g_fail ? 1 : 0;
}

}  // namespace

int main(int argc, char* argv[]) {
    if (argc >= 2 && !strcmp(argv[1], "extract")) return extract_main(argc - 1, argv + 1);
    if (argc >= 2 && !strcmp(argv[1], "synthesis")) return synthesis_main(argc - 1, argv + 1);
    if (argc >= 2 && !strcmp(argv[1], "preref")) return preref_main(argc - 1, argv + 1);
    if (argc >= 2 && !strcmp(argv[1], "seams")) return seams();
    if (argc >= 2 && !strcmp(argv[1], "limits")) return limits();
    fprintf(stderr, "usage: refseq_check extract|synthesis|preref <the program's arguments> | seams | limits\n");
    return 2;
}
