// gmap_check.cpp -- TEST INFRASTRUCTURE: rsem-tbam2gbam without a device.  The program's own host code (rsem_amd/csrc/host/
// gbam_host.hpp: reader, units and groups, fields, record assembly, BGZF out) runs unchanged; the entry points it calls,
// rsem_gmap_create / rsem_gmap_convert / rsem_gmap_destroy, are defined HERE and walk the same steps as rsem_amd/csrc/gmap.hip with the
// same functions of rsem_amd/csrc/gmap_block.hpp: batches, map_mate and fill_cigar per mate, and for every group collapse_group -- the
// kernel's body -- on tests/simt_emu.hpp (one OS thread per lane, "LDS" in memory, the barriers barriers): a wave for a group of up
// to 64 alignments, a workgroup for a longer one.  Built with AddressSanitizer and UBSan (tests/test_gmap_cpu.py).  Never part of
// the product.
//
//   gmap_check convert <reference_name> <alignments> <out.bam> [-p N]     the recorded CL: is that of "rsem-tbam2gbam <the three names>"
//   gmap_check collapse <n> <run>      a group of n alignments in runs of `run` equal keys against std::map, both widths' seams
//   gmap_check fields < text           transcripts and a case (tests/gmap_limits.py: fields_input) -> every mate's fields and words, the kept
//                                      alignments and their weights' bits, the batches
// Build: hipcc (host compilation of the HIP headers simt_emu.hpp pulls in) -DRSEM_EMU -fsanitize=address,undefined -fno-gpu-sanitize
#include "simt_emu.hpp"

#include <map>

#include "../rsem_amd/csrc/gmap_block.hpp"
#include "../rsem_amd/csrc/host/gbam_host.hpp"

using namespace rsem_gmapk;

struct rsem_gmap {
    int32_t n_tr = 0;
    std::vector<uint8_t> minus;
    std::vector<int32_t> length, out_tid, start, end, cum;
    std::vector<uint64_t> exon_off;
    Ref ref() const { return Ref{minus.data(), length.data(), out_tid.data(), exon_off.data(), start.data(), end.data(), cum.data()}; }
};

namespace {

std::string g_error;

struct Job {
    emu::Block blk;
    Key stage[kGroupThreads];  // "LDS"
    uint32_t g0, n;
    int mates, width;
    MateArrays A;
    const float* w;
    const uint32_t* cigar;
    uint32_t *order, *head;
    float* wsum;
};

void lane_body(Job* J, int tid) {
    emu::t_tid = tid;
    emu::t_blk = &J->blk;
    if (J->width == kWave) collapse_group<kWave>(J->g0, J->n, tid & 63, J->mates, J->A, J->w, J->cigar, J->stage, J->order, J->head, J->wsum);
    else collapse_group<kGroupThreads>(J->g0, J->n, tid, J->mates, J->A, J->w, J->cigar, J->stage, J->order, J->head, J->wsum);
}

void run_group(Job* J) {
    J->width = J->n <= (uint32_t)kWave ? kWave : kGroupThreads;
    std::vector<std::thread> th;
    for (int t = 0; t < J->width; t++) th.emplace_back(lane_body, J, t);
    for (auto& t : th) t.join();
}

Job* new_job() {
    static_assert(kGroupThreads == 256 && RSEM_BDIM == 256, "the emulator's workgroup is the kernel's");
    Job* J = new Job();
    pthread_barrier_init(&J->blk.bar, nullptr, 256);
    for (int k = 0; k < 4; k++) pthread_barrier_init(&J->blk.w[k].bar, nullptr, 64);
    return J;
}

}  // namespace

extern "C" const char* rsem_hip_strerror(int) { return "error"; }
extern "C" const char* rsem_hip_last_error(void) { return g_error.c_str(); }

extern "C" int rsem_gmap_create(rsem_gmap** out, int, int32_t n, const uint8_t* strand, const int32_t* length, const int32_t* out_tid, const uint64_t* exon_off,
                                const int32_t* exon_start, const int32_t* exon_end) {
    rsem_gmap* h = new rsem_gmap();
    h->n_tr = n;
    for (int32_t t = 0; t < n; t++) h->minus.push_back(strand[t] == '-');
    h->length.assign(length, length + n);
    h->out_tid.assign(out_tid, out_tid + n);
    h->exon_off.assign(exon_off, exon_off + n + 1);
    h->start.assign(exon_start, exon_start + exon_off[n]);
    h->end.assign(exon_end, exon_end + exon_off[n]);
    h->cum.resize(exon_off[n]);
    for (int32_t t = 0; t < n; t++) {
        int32_t c = 0;
        for (uint64_t e = exon_off[t]; e < exon_off[t + 1]; e++) { h->cum[e] = c; c += exon_end[e] - exon_start[e] + 1; }
        if (c != length[t]) { g_error = "a transcript's exons do not add up to its length"; delete h; return RSEM_ERR_INVALID; }
    }
    *out = h;
    return RSEM_OK;
}

extern "C" void rsem_gmap_destroy(rsem_gmap* h) { delete h; }

extern "C" int rsem_gmap_convert(rsem_gmap* h, int32_t mates, int64_t n_aln, int64_t n_groups, const uint64_t* group_off, const int32_t* tr, const int32_t* pos,
                                 const int32_t* l_qseq, const uint32_t* flag, const float* w, int32_t* out_tid, int32_t* out_pos, uint32_t* out_flag,
                                 uint32_t* out_n_cigar, uint32_t* out_bin, uint32_t* out_has_n, uint64_t* cigar_off, uint32_t* cigar_words, uint64_t cigar_cap,
                                 uint64_t* out_src, float* out_w, rsem_gmap_info* info) {
    uint64_t budget = kDefaultBatchItems;
    if (const char* e = getenv("RSEM_GMAP_BATCH_ITEMS")) budget = (uint64_t)atoll(e);
    if (info) { memset(info, 0, sizeof(*info)); info->batch_items = budget; info->n_groups = (uint64_t)n_groups; info->n_alignments_in = (uint64_t)n_aln; }
    cigar_off[0] = 0;
    if (!n_aln) return RSEM_OK;
    const Ref R = h->ref();
    Job* J = new_job();
    uint64_t words_done = 0, out_done = 0;
    for (uint64_t lo = 0; lo < (uint64_t)n_groups;) {
        const uint64_t hi = batch_end(group_off, (uint64_t)n_groups, lo, budget);
        const uint64_t a_lo = group_off[lo], na = group_off[hi] - a_lo, m_lo = a_lo * (uint64_t)mates, nm = na * (uint64_t)mates;
        // k_gmap_count, the scan, k_gmap_fill: the batch's own arrays, offsets inside the batch
        std::vector<int32_t> b_tid(nm), b_pos(nm);
        std::vector<uint32_t> b_flag(nm), b_nc(nm), b_coff(nm + 1, 0), b_cigar;
        for (uint64_t i = 0; i < nm; i++) {
            const Mapped m = map_mate(R, tr[m_lo + i], pos[m_lo + i], l_qseq[m_lo + i], flag[m_lo + i]);
            b_tid[i] = out_tid[m_lo + i] = m.tid; b_pos[i] = out_pos[m_lo + i] = m.pos; b_flag[i] = out_flag[m_lo + i] = m.flag;
            b_nc[i] = out_n_cigar[m_lo + i] = m.n_cigar; out_bin[m_lo + i] = m.bin; out_has_n[m_lo + i] = m.has_n;
            b_coff[i + 1] = b_coff[i] + m.n_cigar;
        }
        b_cigar.resize(b_coff[nm]);  // exactly: a word too many is a heap overflow the sanitizer reports
        if (words_done + b_cigar.size() > cigar_cap) { g_error = "the CIGARs take more than cigar_cap words"; return RSEM_ERR_INVALID; }
        for (uint64_t i = 0; i < nm; i++) {
            const Mapped m = map_mate(R, tr[m_lo + i], pos[m_lo + i], l_qseq[m_lo + i], flag[m_lo + i]);
            fill_cigar(R, tr[m_lo + i], m, b_cigar.data() + b_coff[i]);
        }
        // k_gmap_collapse: a wave or a workgroup per group
        std::vector<uint32_t> order(na, ~0u), head(na + 1, 0), scan(na + 1, 0);
        std::vector<float> wsum(na, 0.0f);
        J->mates = mates;
        J->A = MateArrays{b_tid.data(), b_pos.data(), b_flag.data(), b_nc.data(), b_coff.data()};
        J->w = w + a_lo; J->cigar = b_cigar.data(); J->order = order.data(); J->head = head.data(); J->wsum = wsum.data();
        for (uint64_t g = lo; g < hi; g++) {
            J->g0 = (uint32_t)(group_off[g] - a_lo);
            J->n = (uint32_t)(group_off[g + 1] - group_off[g]);
            run_group(J);
        }
        // the scan and k_gmap_emit
        for (uint64_t p = 0; p < na; p++) scan[p + 1] = scan[p] + head[p];
        for (uint64_t p = 0; p < na; p++)
            if (head[p]) { out_src[out_done + scan[p]] = a_lo + order[p]; out_w[out_done + scan[p]] = wsum[p]; }
        for (uint64_t i = 0; i <= nm; i++) cigar_off[m_lo + i] = words_done + b_coff[i];
        memcpy(cigar_words + words_done, b_cigar.data(), b_cigar.size() * 4);
        words_done += b_cigar.size();
        out_done += scan[na];
        if (info) info->n_batches++;
        lo = hi;
    }
    delete J;
    if (info) { info->n_alignments_out = out_done; info->n_cigar_words = words_done; }
    return RSEM_OK;
}

int main(int argc, char* argv[]) {
    using namespace rsemh;
    if (argc >= 5 && !strcmp(argv[1], "convert")) {
        GbamOptions opt;
        opt.quiet = true;
        opt.threads = argc == 7 ? atoi(argv[6]) : 3;
        convert_transcript_bam(argv[2], argv[3], argv[4], opt, std::string("rsem-tbam2gbam ") + argv[2] + " " + argv[3] + " " + argv[4]);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "collapse")) {
        // one transcript of 3 exons on '+'; alignment a starts at base (a / run) % 40 of it: runs of `run` equal keys, the keys in no order
        const uint32_t n = (uint32_t)atoi(argv[2]), run = (uint32_t)atoi(argv[3]);
        const uint8_t strand[1] = {'+'};
        const int32_t length[1] = {120}, tid[1] = {2}, st[3] = {100, 200, 300}, en[3] = {139, 239, 339};
        const uint64_t eoff[2] = {0, 3}, goff[2] = {0, n};
        rsem_gmap* h = nullptr;
        if (rsem_gmap_create(&h, 0, 1, strand, length, tid, eoff, st, en) != RSEM_OK) return 2;
        std::vector<int32_t> tr(n, 0), pos(n), lq(n, 50), otid(n), opos(n);
        std::vector<uint32_t> flag(n, 0), of(n), onc(n), ob(n), ohn(n), cig(8 * (size_t)n);
        std::vector<float> w(n), ow(n);
        std::vector<uint64_t> coff(n + 1), osrc(n);
        std::map<int32_t, std::pair<uint64_t, float>> want;  // (on one transcript and strand the key orders as the position does)
        for (uint32_t a = 0; a < n; a++) {
            pos[a] = (int32_t)((a / run) * 7 % 40);
            w[a] = (a % 3 == 0) ? 1.0f : (a % 3 == 1 ? 5.9604645e-8f : 0.1f);
            auto it = want.find(pos[a]);
            if (it == want.end()) want[pos[a]] = {a, w[a]}; else it->second.second += w[a];
        }
        rsem_gmap_info info;
        if (rsem_gmap_convert(h, 1, n, 1, goff, tr.data(), pos.data(), lq.data(), flag.data(), w.data(), otid.data(), opos.data(), of.data(), onc.data(), ob.data(),
                              ohn.data(), coff.data(), cig.data(), cig.size(), osrc.data(), ow.data(), &info) != RSEM_OK) { fprintf(stderr, "%s\n", g_error.c_str()); return 2; }
        rsem_gmap_destroy(h);
        if (info.n_alignments_out != want.size()) { fprintf(stderr, "%llu kept, %zu expected\n", (unsigned long long)info.n_alignments_out, want.size()); return 1; }
        size_t k = 0;
        for (const auto& kv : want) {
            if (osrc[k] != kv.second.first || memcmp(&ow[k], &kv.second.second, 4) != 0) { fprintf(stderr, "output %zu differs\n", k); return 1; }
            k++;
        }
        printf("ok %zu\n", want.size());
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "fields")) {
        unsigned long long n_tr, n_ex, x, y, z, v;
        if (scanf("%llu %llu", &n_tr, &n_ex) != 2) return 2;
        std::vector<uint8_t> strand(n_tr);
        std::vector<int32_t> length(n_tr), tid(n_tr), st(n_ex), en(n_ex);
        std::vector<uint64_t> eoff(n_tr + 1, 0);
        for (size_t t = 0; t < n_tr; t++) {
            if (scanf("%llu %llu %llu %llu", &x, &y, &z, &v) != 4) return 2;
            strand[t] = (uint8_t)x; length[t] = (int32_t)y; tid[t] = (int32_t)z; eoff[t + 1] = v;
        }
        for (size_t e = 0; e < n_ex; e++) {
            if (scanf("%llu %llu", &x, &y) != 2) return 2;
            st[e] = (int32_t)x; en[e] = (int32_t)y;
        }
        unsigned long long mates, n, ng;
        if (scanf("%llu %llu %llu", &mates, &n, &ng) != 3) return 2;
        const size_t nm = n * mates;
        std::vector<uint64_t> goff(ng + 1), coff(nm + 1), osrc(n);
        for (auto& g : goff) { if (scanf("%llu", &x) != 1) return 2; g = x; }
        std::vector<int32_t> tr(nm), pos(nm), lq(nm), otid(nm), opos(nm);
        std::vector<uint32_t> flag(nm), of(nm), onc(nm), ob(nm), ohn(nm);
        std::vector<float> w(n), ow(n);
        size_t cap = 0;
        for (size_t i = 0; i < nm; i++) {
            if (scanf("%llu %llu %llu %llu", &x, &y, &z, &v) != 4 || x >= n_tr) return 2;
            tr[i] = (int32_t)x; pos[i] = (int32_t)y; lq[i] = (int32_t)z; flag[i] = (uint32_t)v;
            cap += 2 * (eoff[x + 1] - eoff[x]) + 2;  // the bound include/rsem_hip.h states
        }
        for (size_t a = 0; a < n; a++) {
            unsigned b;
            if (scanf("%x", &b) != 1) return 2;
            memcpy(&w[a], &b, 4);
        }
        std::vector<uint32_t> cig(cap);
        rsem_gmap* h = nullptr;
        if (rsem_gmap_create(&h, 0, (int32_t)n_tr, strand.data(), length.data(), tid.data(), eoff.data(), st.data(), en.data()) != RSEM_OK) {
            fprintf(stderr, "%s\n", g_error.c_str());
            return 2;
        }
        rsem_gmap_info info;
        if (rsem_gmap_convert(h, (int32_t)mates, (int64_t)n, (int64_t)ng, goff.data(), tr.data(), pos.data(), lq.data(), flag.data(), w.data(), otid.data(), opos.data(),
                              of.data(), onc.data(), ob.data(), ohn.data(), coff.data(), cig.data(), cig.size(), osrc.data(), ow.data(), &info) != RSEM_OK) {
            fprintf(stderr, "%s\n", g_error.c_str());
            return 2;
        }
        rsem_gmap_destroy(h);
        for (size_t i = 0; i < nm; i++) {
            printf("%d %d %u %u %u %u", otid[i], opos[i], of[i], onc[i], ob[i], ohn[i]);
            for (uint64_t k = coff[i]; k < coff[i + 1]; k++) printf(" %u", cig[k]);
            printf("\n");
        }
        for (uint64_t k = 0; k < info.n_alignments_out; k++) {
            unsigned b;
            memcpy(&b, &ow[k], 4);
            printf("out %llu %08x\n", (unsigned long long)osrc[k], b);
        }
        fprintf(stderr, "batches %d\n", info.n_batches);
        return 0;
    }
    fprintf(stderr, "usage: gmap_check convert|collapse|fields ...\n");
    return 2;
}
