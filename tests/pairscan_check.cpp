// pairscan_check.cpp -- TEST INFRASTRUCTURE: rsem-scan-for-paired-end-reads without a device.  The program's own host code
// (rsem_amd/csrc/host/pairscan_host.hpp: reader, held-back run, fields, messages, gather, BGZF out) runs unchanged; the entry points it
// calls, rsem_pairscan_create / _reorder / _destroy, are defined HERE and walk the same steps as rsem_amd/csrc/pairscan.hip with the same
// functions of rsem_amd/csrc/pairscan_block.hpp: batches, and per batch mark_record, the scans as loops (RunCount with the operator
// itself), opens_group, place_body -- which reduces across a wave -- and rank_group, by a wave and by a workgroup, on tests/simt_emu.hpp
// (one OS thread per lane).  Every buffer has exactly the size the device code relies on: a byte too far is a heap overflow the
// sanitizer reports.  Built with AddressSanitizer and UBSan (tests/test_pairscan_cpu.py).  Never part of the product.
//
//   pairscan_check <N> <alignments> <out.bam>
//   pairscan_check records <file>      rsem_pairscan_reorder on records given as text, the verdict and the permutation printed
// Build: hipcc (host compilation of the HIP headers simt_emu.hpp pulls in) -DRSEM_EMU -fsanitize=address,undefined -fno-gpu-sanitize
#include "simt_emu.hpp"

#include "../rsem_amd/csrc/pairscan_block.hpp"
#include "../rsem_amd/csrc/host/pairscan_host.hpp"

using namespace rsem_pairk;

struct rsem_pairscan {
    bool ended = false;
};

namespace {

std::string g_error;

emu::Block& block() {
    static emu::Block blk;
    static bool init = false;
    if (!init) {
        emu::barrier_init(&blk.bar, 256);
        for (int k = 0; k < 4; k++) emu::barrier_init(&blk.w[k].bar, 64);
        init = true;
    }
    return blk;
}

// a workgroup of `threads` lanes (whole waves): body(thread)
template <class F>
void workgroup(int threads, const F& body) {
    emu::Block& blk = block();
    std::vector<std::thread> th;
    for (int t = 0; t < threads; t++)
        th.emplace_back([&, t] {
            emu::t_tid = t;
            emu::t_blk = &blk;
            body(t);
        });
    for (auto& t : th) t.join();
}

// a launch of ceil(n / 64) waves (the last lanes idle, as on the device): body(live, index)
template <class F>
void launch(uint64_t n, const F& body) {
    for (uint64_t b0 = 0; b0 < n; b0 += 256) {
        const int waves = (int)std::min<uint64_t>(4, (n - b0 + 63) / 64);
        workgroup(waves * 64, [&](int t) { body(b0 + (uint64_t)t < n, b0 + (uint64_t)t); });
    }
}

}  // namespace

extern "C" const char* rsem_hip_strerror(int) { return "error"; }
extern "C" const char* rsem_hip_last_error(void) { return g_error.c_str(); }

extern "C" int rsem_pairscan_create(rsem_pairscan** out, int) {
    *out = new rsem_pairscan();
    return RSEM_OK;
}

extern "C" void rsem_pairscan_destroy(rsem_pairscan* h) { delete h; }

extern "C" int rsem_pairscan_reorder(rsem_pairscan* h, int64_t n_records, const uint64_t* name_off, const uint8_t* names, const uint32_t* flag, const int32_t* tid,
                                     const int32_t* pos, const int32_t* mpos, int32_t last, uint32_t* perm_out, rsem_pairscan_verdict* v) {
    uint64_t budget = kDefaultBatchItems;
    if (const char* e = getenv("RSEM_PAIRSCAN_BATCH_ITEMS")) budget = (uint64_t)atoll(e);
    if (h->ended) { g_error = "the call before this one was the last"; return RSEM_ERR_STATE; }
    memset(v, 0, sizeof(*v));
    v->group = v->group_record = -1;
    v->n_records = (uint64_t)n_records;
    if (n_records == 0) { h->ended = last != 0; return RSEM_OK; }
    for (int64_t i = 0; i < n_records; i++)
        if (name_off[i + 1] <= name_off[i] || name_off[i + 1] - name_off[i] > kMaxName) { g_error = "a record's name"; return RSEM_ERR_INVALID; }
    const Recs all{name_off, names, 0, flag, tid, pos, mpos, n_records};
    unsigned long long word = kNoVerdict;
    uint64_t group_base = 0;
    for (uint64_t lo = 0; lo < (uint64_t)n_records && word == kNoVerdict;) {
        const uint64_t hi = batch_end(all, lo, budget), n = hi - lo;
        // the batch's own copies, as uploaded
        std::vector<uint64_t> b_noff(name_off + lo, name_off + hi + 1);
        std::vector<uint8_t> b_names(names + name_off[lo], names + name_off[hi]);
        std::vector<uint32_t> b_flag(flag + lo, flag + hi);
        std::vector<int32_t> b_tid(tid + lo, tid + hi), b_pos(pos + lo, pos + hi), b_mpos(mpos + lo, mpos + hi);
        const Recs R{b_noff.data(), b_names.data(), name_off[lo], b_flag.data(), b_tid.data(), b_pos.data(), b_mpos.data(), (int64_t)n};
        std::vector<uint32_t> mark(n), run(n), open(n), ord(n), perm(n), both_src(n);
        std::vector<uint64_t> wa(n + 1, 0), wb(n + 1, 0), ca(n + 1, 0), cb(n + 1, 0), sw(n + 1, 0), sws(n + 1, 0);
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t c = class_of(R.flag[i]);
            mark[i] = mark_record(R, (int64_t)i);
            wa[i] = class_word_a(c);
            wb[i] = class_word_b(c);
        }
        run[0] = mark[0];
        for (uint64_t i = 1; i < n; i++) run[i] = RunCount()(run[i - 1], mark[i]);
        for (uint64_t i = 0; i < n; i++) { ca[i + 1] = ca[i] + wa[i]; cb[i + 1] = cb[i] + wb[i]; }
        uint32_t ng = 0;
        for (uint64_t i = 0; i < n; i++) { open[i] = opens_group(mark[i], run[i]); ord[i] = ng += open[i]; }
        std::vector<uint32_t> goff(ng + 1);  // exactly
        for (uint64_t i = 0; i < n; i++)
            if (open[i]) goff[ord[i] - 1] = (uint32_t)i;
        goff[ng] = (uint32_t)n;
        const Scans S{ord.data(), ca.data(), cb.data()};
        launch(n, [&](bool live, uint64_t i) {
            place_body(live, (int64_t)i, R, S, goff.data(), group_base, (uint32_t)lo, perm.data(), both_src.data(), sw.data(), &word);
        });
        for (uint64_t i = 0; i < n; i++) sws[i + 1] = sws[i] + sw[i];
        const uint32_t n_small = (uint32_t)(sws[n] & 0xffffffffull), n_large = (uint32_t)(sws[n] >> 32);
        std::vector<uint32_t> small(n_small), large(n_large);  // exactly
        for (uint64_t i = 0; i < n; i++) {
            if (!sw[i]) continue;
            if (sw[i] & 0xffffffffull) small[sws[i] & 0xffffffffull] = ord[i] - 1;
            else large[sws[i] >> 32] = ord[i] - 1;
        }
        if (word == kNoVerdict) {
            for (uint32_t b = 0; b < (n_small + 3) / 4 + n_large; b++) {  // k_pairscan_rank, block by block
                Key stage[kGroupThreads];
                const uint32_t nb_small = (n_small + 3) / 4;
                workgroup(kGroupThreads, [&](int t) {
                    if (b < nb_small) {
                        const int wv = t >> 6;
                        const uint32_t idx = b * 4u + (uint32_t)wv;
                        if (idx >= n_small) return;
                        const uint32_t g = small[idx], g0 = goff[g];
                        rank_group<kWave>(g0, (uint32_t)((ca[goff[g + 1]] - ca[g0]) & 0xffffffffull), t & 63, R, both_src.data(), stage + wv * kWave, (uint32_t)lo, perm.data());
                    } else {
                        const uint32_t g = large[b - nb_small], g0 = goff[g];
                        rank_group<kGroupThreads>(g0, (uint32_t)((ca[goff[g + 1]] - ca[g0]) & 0xffffffffull), t, R, both_src.data(), stage, (uint32_t)lo, perm.data());
                    }
                });
            }
            memcpy(perm_out + lo, perm.data(), n * 4);
        } else v->group_record = (int64_t)(lo + goff[(word >> 8) - group_base]);
        v->n_batches++;
        v->n_sorted_groups += n_small + n_large;
        group_base += ng;
        lo = hi;
    }
    v->n_groups = group_base;
    if (word != kNoVerdict) {
        v->code = (int32_t)(word & 0xffu);
        v->group = (int64_t)(word >> 8);
    } else h->ended = last != 0;
    return RSEM_OK;
}

// records <file>: the arrays of rsem_pairscan_reorder as text, a record a line -- the name in hexadecimal, flag, tid, pos, mpos -- for what
// no alignment file carries (a NUL inside a name, a tid at the ends of 32 bits).  Prints the verdict's words, then the permutation.
int records_main(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<uint64_t> name_off{0};
    std::vector<uint8_t> names;
    std::vector<uint32_t> flag;
    std::vector<int32_t> tid, pos, mpos;
    char hex[2 * 300];
    long long fl, t, p, m;
    while (fscanf(f, "%599s %lld %lld %lld %lld", hex, &fl, &t, &p, &m) == 5) {
        for (size_t k = 0; hex[k] && hex[k + 1]; k += 2) {
            unsigned v = 0;
            sscanf(hex + k, "%2x", &v);
            names.push_back((uint8_t)v);
        }
        name_off.push_back(names.size());
        flag.push_back((uint32_t)fl); tid.push_back((int32_t)t); pos.push_back((int32_t)p); mpos.push_back((int32_t)m);
    }
    fclose(f);
    names.shrink_to_fit();  // exactly the names' bytes: a read behind them is a heap overflow
    rsem_pairscan* h = nullptr;
    rsem_pairscan_create(&h, 0);
    std::vector<uint32_t> perm(flag.size());
    rsem_pairscan_verdict v;
    const int rc = rsem_pairscan_reorder(h, (int64_t)flag.size(), name_off.data(), names.data(), flag.data(), tid.data(), pos.data(), mpos.data(), 1, perm.data(), &v);
    rsem_pairscan_destroy(h);
    if (rc) { fprintf(stderr, "rsem_pairscan_reorder: %d (%s)\n", rc, g_error.c_str()); return 1; }
    printf("%d %lld %lld %llu %d %llu\n", v.code, (long long)v.group, (long long)v.group_record, (unsigned long long)v.n_groups, v.n_batches, (unsigned long long)v.n_sorted_groups);
    if (!v.code)
        for (uint32_t x : perm) printf("%u\n", x);
    return 0;
}

int main(int argc, char* argv[]) {
    using namespace rsemh;
    if (argc == 3 && !strcmp(argv[1], "records")) return records_main(argv[2]);
    if (argc != 4) {
        fprintf(stderr, "usage: pairscan_check <N> <alignments> <out.bam> | records <file>\n");
        return 2;
    }
    AlncheckOptions opt;
    opt.threads = std::max(1, atoi(argv[1]));
    scan_for_paired_end_reads(argv[2], argv[3], opt);
    return 0;
}
