// alncheck_check.cpp -- TEST INFRASTRUCTURE: rsem-sam-validator and rsem-get-unique without a device.  The programs' own host code
// (rsem_amd/csrc/host/alncheck_host.hpp: reader, fields, messages, BGZF out) runs unchanged; the entry points it calls,
// rsem_alncheck_create / _push / _destroy / _unique, are defined HERE and walk the same steps as rsem_amd/csrc/alncheck.hip with the same
// functions of rsem_amd/csrc/alncheck_block.hpp: batches, and per batch unit_body and lookup_body -- the kernels' bodies, which reduce
// across a wave -- on tests/simt_emu.hpp (one OS thread per lane), the scan as a loop, the radix sort as std::stable_sort.  Every
// buffer has exactly the size the device code relies on: a byte too far is a heap overflow the sanitizer reports.  Built with
// AddressSanitizer and UBSan (tests/test_alncheck_cpu.py).  Never part of the product.
//
//   alncheck_check validate <alignments> [-p N]
//   alncheck_check unique <N> <alignments> <out.bam>
// Build: hipcc (host compilation of the HIP headers simt_emu.hpp pulls in) -DRSEM_EMU -fsanitize=address,undefined -fno-gpu-sanitize
#include "simt_emu.hpp"

#include "../rsem_amd/csrc/alncheck_block.hpp"
#include "../rsem_amd/csrc/host/alncheck_host.hpp"

using namespace rsem_alnk;

struct rsem_alncheck {
    std::vector<uint32_t> target_len;
    int paired = -1;
    bool refused = false;
    Carry carry[2];
    int cur = 0;
    std::vector<uint64_t> res_hash, res_ref, run_off{0};
    std::vector<uint8_t> res_names;
    rsem_alncheck() { memset(carry, 0, sizeof(carry)); }
};

namespace {

std::string g_error;

// a launch of ceil(n / 64) waves (the last lanes idle, as on the device): body(live, index) on a thread per lane
template <class F>
void launch(uint64_t n, const F& body) {
    static emu::Block blk;
    static bool init = false;
    if (!init) {
        for (int k = 0; k < 4; k++) emu::barrier_init(&blk.w[k].bar, 64);
        init = true;
    }
    for (uint64_t b0 = 0; b0 < n; b0 += 256) {
        const int waves = (int)std::min<uint64_t>(4, (n - b0 + 63) / 64);
        std::vector<std::thread> th;
        for (int t = 0; t < waves * 64; t++)
            th.emplace_back([&, t] {
                emu::t_tid = t;
                emu::t_blk = &blk;
                body(b0 + (uint64_t)t < n, b0 + (uint64_t)t);
            });
        for (auto& t : th) t.join();
    }
}

void knobs(uint64_t& budget, int& bits) {
    budget = kDefaultBatchItems;
    bits = 64;
    if (const char* e = getenv("RSEM_ALNCHECK_BATCH_ITEMS")) budget = (uint64_t)atoll(e);
    if (const char* e = getenv("RSEM_ALNCHECK_HASH_BITS")) bits = atoi(e);
}

}  // namespace

extern "C" const char* rsem_hip_strerror(int) { return "error"; }
extern "C" const char* rsem_hip_last_error(void) { return g_error.c_str(); }

extern "C" int rsem_alncheck_create(rsem_alncheck** out, int, int32_t n, const uint32_t* target_len) {
    rsem_alncheck* h = new rsem_alncheck();
    h->target_len.assign(target_len, target_len + n);
    *out = h;
    return RSEM_OK;
}

extern "C" void rsem_alncheck_destroy(rsem_alncheck* h) { delete h; }

extern "C" int rsem_alncheck_push(rsem_alncheck* h, int64_t n, const uint64_t* name_off, const uint8_t* names, const uint32_t* flag, const int32_t* tid, const int32_t* pos,
                                  const int32_t* isize, const int32_t* lq, const uint64_t* cigar_off, const uint32_t* cigar, int32_t last, rsem_alncheck_verdict* v) {
    uint64_t budget;
    int bits;
    knobs(budget, bits);
    if (h->refused) { g_error = "a verdict has been returned"; return RSEM_ERR_STATE; }
    memset(v, 0, sizeof(*v));
    v->unit_record = -1;
    if (n == 0) return RSEM_OK;
    for (int64_t i = 0; i < n; i++) {
        if (name_off[i + 1] <= name_off[i] || name_off[i + 1] - name_off[i] > kMaxName || is_space(names[name_off[i]])) { g_error = "a record's name"; return RSEM_ERR_INVALID; }
        if (lq[i] < 1 || (!(flag[i] & 4u) && (tid[i] < 0 || tid[i] >= (int32_t)h->target_len.size()))) { g_error = "a record's l_qseq or tid"; return RSEM_ERR_INVALID; }
    }
    if (h->paired < 0) h->paired = (int)(flag[0] & 1u);
    if (h->paired && !last && (n & 1)) { g_error = "an odd number of paired-end records"; return RSEM_ERR_INVALID; }
    const int mates = h->paired ? 2 : 1;
    unsigned long long word = kNoVerdict;
    uint32_t fail_detail = 0;
    for (uint64_t lo = 0; lo < (uint64_t)n && word == kNoVerdict;) {
        const uint64_t nrec = batch_records((uint64_t)n - lo, budget, mates), nu = (nrec + mates - 1) / mates, unit_base = lo / mates;
        // the batch's own copies, as uploaded
        std::vector<uint64_t> b_noff(name_off + lo, name_off + lo + nrec + 1), b_coff(cigar_off + lo, cigar_off + lo + nrec + 1);
        std::vector<uint8_t> b_names(names + name_off[lo], names + name_off[lo + nrec]);
        std::vector<uint32_t> b_flag(flag + lo, flag + lo + nrec), b_cigar(cigar + cigar_off[lo], cigar + cigar_off[lo + nrec]);
        std::vector<int32_t> b_tid(tid + lo, tid + lo + nrec), b_pos(pos + lo, pos + lo + nrec), b_isize(isize + lo, isize + lo + nrec), b_lq(lq + lo, lq + lo + nrec);
        const Recs R{b_noff.data(), b_names.data(), name_off[lo], b_flag.data(), b_tid.data(), b_pos.data(), b_isize.data(), b_lq.data(), b_coff.data(), b_cigar.data(),
                     cigar_off[lo], (int64_t)nrec};
        std::vector<uint32_t> detail(nu), g_unit(nu), s_unit(nu);
        std::vector<uint64_t> hash(nu), open(nu + 1, 0), scan(nu + 1, 0), g_hash(nu), u_ref(nu);
        const UnitArrays A{detail.data(), hash.data(), open.data()};
        const Carry* before = &h->carry[h->cur];
        Carry* after = &h->carry[h->cur ^ 1];
        launch(nu, [&](bool live, uint64_t u) {
            unit_body(live, (int64_t)u, R, h->paired, h->target_len.data(), before, after, (int64_t)nu, bits, unit_base, A, &word);
        });
        for (uint64_t u = 0; u < nu; u++) scan[u + 1] = scan[u] + open[u];
        const uint64_t ng = scan[nu] >> 40, name_bytes = scan[nu] & ((1ull << 40) - 1ull);
        const uint64_t G0 = h->res_hash.size(), N0 = h->res_names.size();
        h->res_names.resize(N0 + name_bytes);  // exactly
        h->res_hash.resize(G0 + ng);
        h->res_ref.resize(G0 + ng);
        for (uint64_t u = 0; u < nu; u++) gather_unit((int64_t)u, R, mates, open.data(), scan.data(), hash.data(), N0, h->res_names.data(), g_hash.data(), g_unit.data(), u_ref.data());
        if (ng) {
            std::vector<uint32_t> order(ng);
            for (uint32_t g = 0; g < ng; g++) order[g] = g;
            std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return g_hash[a] < g_hash[b]; });
            for (uint64_t p = 0; p < ng; p++) { h->res_hash[G0 + p] = g_hash[order[p]]; s_unit[p] = g_unit[order[p]]; }
            const Resident S{h->res_hash.data(), h->res_ref.data(), h->res_names.data(), h->run_off.data(), (uint32_t)(h->run_off.size() - 1)};
            launch(ng, [&](bool live, uint64_t p) { lookup_body(live, p, S, s_unit.data(), u_ref.data(), detail.data(), unit_base, &word); });
            h->run_off.push_back(G0 + ng);
        }
        v->n_batches++;
        if (word != kNoVerdict) fail_detail = detail[(word >> 8) - unit_base];
        else h->cur ^= 1;
        lo += nrec;
    }
    const uint64_t n_units = ((uint64_t)n + mates - 1) / mates;
    v->n_units = n_units;
    v->resident_groups = h->res_hash.size();
    v->resident_name_bytes = h->res_names.size();
    if (word != kNoVerdict) {
        h->refused = true;
        v->code = (int32_t)(fail_detail & 0xffu);
        v->mate = (int32_t)((fail_detail >> 8) & 0xffu);
        v->cigar_op = fail_detail >> 16;
        v->units_ok = word >> 8;
        v->unit_record = (int64_t)((word >> 8) * (uint64_t)mates);
    } else v->units_ok = n_units;
    return RSEM_OK;
}

extern "C" int rsem_alncheck_unique(int, int64_t n, const uint64_t* name_off, const uint8_t* names, const uint32_t* flag, uint8_t* keep, rsem_alncheck_info* info) {
    uint64_t budget;
    int bits;
    knobs(budget, bits);
    if (info) memset(info, 0, sizeof(*info));
    for (uint64_t lo = 0; lo < (uint64_t)n;) {
        uint64_t hi = std::min<uint64_t>((uint64_t)n, lo + budget);
        while (hi < (uint64_t)n && name_off[hi + 1] - name_off[hi] == name_off[hi] - name_off[hi - 1] &&
               !memcmp(names + name_off[hi], names + name_off[hi - 1], name_off[hi] - name_off[hi - 1])) hi++;
        const uint64_t m = hi - lo;
        std::vector<uint64_t> b_noff(name_off + lo, name_off + hi + 1);
        std::vector<uint8_t> b_names(names + name_off[lo], names + name_off[hi]);
        std::vector<uint32_t> b_flag(flag + lo, flag + hi), start(m), incl(m);
        const Recs R{b_noff.data(), b_names.data(), name_off[lo], b_flag.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, (int64_t)m};
        for (uint64_t i = 0; i < m; i++) start[i] = unique_start(R, (int64_t)i);
        uint32_t s = 0;
        for (uint64_t i = 0; i < m; i++) incl[i] = s += start[i];
        for (uint64_t i = 0; i < m; i++) keep[lo + i] = unique_keep(incl.data(), b_flag.data(), (int64_t)m, (int64_t)i);
        if (info) { info->n_batches++; info->n_groups += s; }
        lo = hi;
    }
    return RSEM_OK;
}

int main(int argc, char* argv[]) {
    using namespace rsemh;
    AlncheckOptions opt;
    if (argc >= 3 && !strcmp(argv[1], "validate")) {
        opt.threads = argc == 5 ? atoi(argv[4]) : 3;
        validate_alignments(argv[2], opt);
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "unique")) {
        opt.threads = std::max(1, atoi(argv[2]));
        write_unique(argv[3], argv[4], opt);
        return 0;
    }
    fprintf(stderr, "usage: alncheck_check validate <alignments> [-p N] | unique <N> <alignments> <out.bam>\n");
    return 2;
}
