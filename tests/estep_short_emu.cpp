// estep_short_emu.cpp -- TEST INFRASTRUCTURE: the short classes of the sliced layout (sell_shape.hpp: Shape::cut -- the last value
// plane of a slice stored without its empty quarters) on the CPU.  Two modes:
//
//   estep_short_emu --table       the class table and the index helpers, for every read length 1..256: one line per length
//                                 "L lg K q cut Gk entries" with every class enabled, then "ok" / a line starting with "BAD"
//                                 (entries >= L, every alignment has a place of its own inside the slice's stride, ids 0..83 mean
//                                 what they always meant, shape_of_id inverts the id arithmetic)
//   estep_short_emu in.bin out.bin
//       runs rsem_amd/csrc/estep_block.hpp as tests/estep_emu.cpp does (simt_emu.hpp: one OS thread per lane), on a layout built HERE
//       with the classes on: row_key_of with the mask short_classes_worth_it chose from the histogram of row lengths.
//       in:  i32 M, N1, T, min_units (0: classes off = the layout of simt_emu.hpp; -1: every class on, however thin), q32 (0/1), range_bits, pad, pad; f64 N0
//            u64 row_ptr[N1+1]; i32 sid[nnz]; f64 cp[nnz]; f64 ncp[N1]; f64 theta[M+1]
//       out: f64 counts[M+1], f64 noise total, f64 reads with a non-zero normaliser
//       stdout: "shape fmt lg K cut rows" per shape, "entries N", "mask 0x...", "roundtrip ok|BAD" (F64 planes read back by
//       sell_unfill_row == the CSR that went in, bit for bit)
// Build (tests/test_estep_short_emu_cpu.py): hipcc -DRSEM_EMU tests/estep_short_emu.cpp -lpthread
#include "simt_emu.hpp"

namespace {
using rsem::kEpsilon;
constexpr int kTotSlots = 64;
constexpr int kWindow = 2048;
#include "../rsem_amd/csrc/estep_block.hpp"
}  // namespace

static int table_mode() {
    int bad = 0;
    for (int id = 0; id < kFullShapes; id++) {  // the ids every layout before the classes was built of
        int fmt, lg, K, cut;
        if (!shape_of_id(id, fmt, lg, K, cut) || fmt != id / kShapesPerFmt || lg != (id % kShapesPerFmt) / 4 || K != id % 4 + 1 || cut != 0) {
            printf("BAD id %d decodes to fmt %d lg %d K %d cut %d\n", id, fmt, lg, K, cut);
            ++bad;
        }
    }
    bool seen[kShortPerFmt] = {};
    for (int L = 1; L <= 256; L++) {
        const int id0 = shape_id_of((uint64_t)L), id = shape_id_of((uint64_t)L, 0xffffffffu);
        int fmt, lg, K, cut, fmt0, lg0, K0, cut0;
        if (!shape_of_id(id, fmt, lg, K, cut) || !shape_of_id(id0, fmt0, lg0, K0, cut0)) { printf("BAD L %d: id %d / %d\n", L, id0, id); ++bad; continue; }
        Shape S{};
        S.lg = lg; S.K = K; S.cut = cut; S.fmt = kFmtF64;
        const int G = shape_G(S), Gk = shape_Gk(S), q = 4 - cut;
        const int entries = (K - 1) * G + Gk;  // per read
        printf("%d %d %d %d %d %d %d\n", L, lg, K, q, cut, Gk, entries);
        if (fmt != kFmtF64 || lg != lg0 || K != K0 || cut0 != 0 || full_shape_of_id(id) != id0) { printf("BAD L %d: class (%d %d) of another shape than (%d %d)\n", L, lg, K, lg0, K0); ++bad; }
        if (entries < L) { printf("BAD L %d: %d entries\n", L, entries); ++bad; }
        if (cut && entries - L >= std::max(1, G / 4)) { printf("BAD L %d: %d entries, a smaller class would do\n", L, entries); ++bad; }
        if (id >= kFullShapes) {
            seen[id - kFullShapes] = true;
            if (short_class_index(lg, K, q) != id - kFullShapes) { printf("BAD L %d: class index\n", L); ++bad; }
            if (shape_id_in_fmt(id, kFmtQ32) != id + kShortPerFmt || shape_fmt_of_id(id + kShortPerFmt) != kFmtQ32) { printf("BAD L %d: Q32 twin\n", L); ++bad; }
        }
        {   // the Q32 format rounds q up to 2 or 4: strides of whole 128-byte lines
            int f2, lg2, K2, cut2;
            const int idq = shape_id_of((uint64_t)L, 0xffffffffu, true);
            if (!shape_of_id(idq, f2, lg2, K2, cut2) || lg2 != lg || K2 != K || (cut2 != 0 && cut2 != 2) || cut2 > cut ||
                (K2 - 1) * G + shape_Gk(lg2, cut2) < L || (shape_val_stride(K2, cut2) * 4) % 128 != 0) { printf("BAD L %d: Q32 class cut %d\n", L, cut2); ++bad; }
        }
        // every alignment of every row slot has a place of its own, inside the stride
        const uint32_t R = shape_R(S), stride = shape_val_stride(S);
        std::vector<int> taken(stride, 0);
        for (uint32_t r = 0; r < R; r++)
            for (int c = 0; c < L; c++) {
                bool ok = false;
                const uint32_t off = shape_val_off(S, r, c, &ok);
                if (!ok || off >= stride || taken[off]++) { printf("BAD L %d: slot %u alignment %d -> entry %u\n", L, r, c, off); ++bad; }
            }
        if (stride != (uint32_t)(K * 64 - 16 * cut) || (uint32_t)entries * R != stride) { printf("BAD L %d: stride %u\n", L, stride); ++bad; }
    }
    for (int i = 0; i < kShortPerFmt; i++)
        if (!seen[i]) { printf("BAD class %d is never chosen\n", i); ++bad; }
    if (kMaxShapes > kLongShape || kFullShapes + 2 * kShortPerFmt != kMaxShapes) { printf("BAD id space\n"); ++bad; }
    printf(bad ? "BAD\n" : "ok\n");
    return bad ? 1 : 0;
}

// the layout with the classes: simt_emu.hpp's build_layout (whole rows only), ids decoded by shape_of_id, values placed by the
// helpers of sell_shape.hpp (inside sell_fill_row)
static uint64_t build_layout_short(HostLayout& H, int M, uint64_t N1, const uint64_t* rp, const int32_t* sid, const double* cp, const double* ncp,
                                   bool q32, int range_bits, int min_units, uint64_t* n_entries) {
    unsigned long long hist[2 * kLenHist] = {};
    for (uint64_t i = 0; i < N1; i++) {  // k_row_length_hist
        const uint64_t fr = rp[i], to = rp[i + 1];
        if (to - fr > 256) continue;
        const int fmt = (q32 && row_takes_q32(cp, fr, to, range_bits)) ? kFmtQ32 : kFmtF64;
        hist[fmt * kLenHist + (to - fr)]++;
    }
    const uint64_t mask = min_units > 0 ? short_classes_worth_it(hist, 1, H.T, min_units) : (min_units < 0 ? ~0ull : 0ull);
    std::vector<std::pair<uint64_t, uint32_t>> keyed(N1);
    for (uint64_t i = 0; i < N1; i++) {
        int err = 0;
        const uint64_t key = row_key_of(i, M, rp, sid, q32 ? cp : nullptr, range_bits, kLayoutWindow, &err, 0, nullptr, mask);
        if (err || (int)(key >> (64 - kShapeBits)) == kLongShape) { fprintf(stderr, "estep_short_emu: bad CSR / long row\n"); exit(2); }
        keyed[i] = {key, (uint32_t)i};
    }
    std::stable_sort(keyed.begin(), keyed.end());
    H.order.resize(N1);
    for (uint64_t p = 0; p < N1; p++) H.order[p] = keyed[p].second;
    uint64_t n_planes = 0, val_bytes = 0;
    uint32_t n_slots = 0;
    *n_entries = 0;
    for (uint64_t p = 0; p < N1;) {
        const int id = (int)(keyed[p].first >> (64 - kShapeBits));
        uint64_t e = p;
        while (e < N1 && (int)(keyed[e].first >> (64 - kShapeBits)) == id) ++e;
        Shape S{};
        int fmt, lg, K, cut;
        if (!shape_of_id(id, fmt, lg, K, cut)) { fprintf(stderr, "estep_short_emu: shape id %d\n", id); exit(2); }
        S.fmt = fmt; S.lg = lg; S.K = K; S.cut = cut;
        S.row_base = (uint32_t)p;
        S.n_rows = (uint32_t)(e - p);
        const uint32_t rps = shape_R(S);
        S.n_slices = (S.n_rows + rps - 1) / rps;
        S.slice_base = H.n_slices;
        S.plane_base = n_planes;
        S.slot_base = n_slots;
        S.val_base = val_bytes;
        H.n_slices += S.n_slices;
        n_planes += (uint64_t)S.n_slices * S.K;
        n_slots += S.n_slices * rps;
        val_bytes += shape_val_bytes(S);
        *n_entries += (uint64_t)S.n_slices * shape_val_stride(S);
        H.shapes.push_back(S);
        p = e;
    }
    H.ssid.assign(n_planes * 64, 0);
    H.sval.assign(val_bytes + 8, 0);
    H.sncp.assign(n_slots + 1, 0.0);
    H.sexp.assign(n_slots + 1, 0);
    H.n_slots = n_slots;
    H.x_slot_base = n_slots;
    for (const Shape& S : H.shapes)
        for (uint32_t q = 0; q < S.n_rows; q++) {
            int err = 0;
            sell_fill_row<true>(S, H.T, S.row_base + q, H.order.data(), rp, sid, cp, ncp, H.ssid.data(), H.sval.data(), H.sncp.data(), H.sexp.data(), &err);
            if (err) { fprintf(stderr, "estep_short_emu: sell_fill_row error %d\n", err); exit(2); }
        }
    H.masks.assign(H.n_slices, 0);
    for (const Shape& S : H.shapes)
        for (uint32_t sl = 0; sl < S.n_slices; sl++) {
            unsigned long long m = 0, full = 0;
            for (int l = 0; l < 64; l++)
                if (slice_lane_changed(S, H.T, sl, l, H.ssid.data())) m |= 1ull << l;
            for (int l = 0; l < 64; l++)
                if (m & read_lanes_of(S, l)) full |= 1ull << l;
            H.masks[S.slice_base + sl] = full;
        }
    return mask;
}

struct Job {
    const HostLayout* H;
    Shape S;
    uint32_t slice_begin, n_slices;
    int base, span, M;
    const double* theta;
    double* counts;
    double* tot_noise;
    double* tot_neff;
    double th_win[kWindow], cnt_win[kWindow];
    emu::Block blk;
};

static void lane_body(Job* J, int tid) {
    emu::t_tid = tid;
    emu::t_blk = &J->blk;
    const int lane = tid & 63, w = tid >> 6;
    const HostLayout& H = *J->H;
    const Shape& S = J->S;
    const uint32_t u_end = S.slice_base + J->slice_begin + J->n_slices;
    const uint32_t s_begin = S.slice_base + J->slice_begin + (uint32_t)w * H.T;
    const uint32_t s_end = std::min(u_end, s_begin + H.T);
    double noise = 0.0, neff = 0.0;
#define EMU_BLOCK(KK, QQ)                                                                                                                 \
    estep_block<KK, false, QQ, 2, false>(S, s_begin, s_end, lane, J->base, J->span, J->theta, J->theta, 0.0, J->th_win, J->cnt_win, H.sval.data(), \
                                         H.sexp.data(), H.ssid.data(), H.sncp.data(), H.masks.data(), J->counts, noise, neff, J->M)
    const int code = (S.K - 1) | ((S.fmt == kFmtQ32 ? 1 : 0) << 2);
    if (s_begin < u_end) switch (code) {
        case 0: EMU_BLOCK(1, false); break;
        case 1: EMU_BLOCK(2, false); break;
        case 2: EMU_BLOCK(3, false); break;
        case 3: EMU_BLOCK(4, false); break;
        case 4: EMU_BLOCK(1, true); break;
        case 5: EMU_BLOCK(2, true); break;
        case 6: EMU_BLOCK(3, true); break;
        default: EMU_BLOCK(4, true); break;
    } else {
        const ThetaSrc th = theta_src<false>(J->theta, J->theta, 0.0, lane);
        stage_windows<false>(J->base, J->span, J->M, th, J->th_win, J->cnt_win);
    }
#undef EMU_BLOCK
    RSEM_SYNC();
    for (int i = tid; i < J->span; i += 256)
        if (J->cnt_win[i] != 0.0) emu::atomic_add(&J->counts[J->base + i], J->cnt_win[i]);
    emu::atomic_add(J->tot_noise, noise);
    emu::atomic_add(J->tot_neff, neff);
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--table")) return table_mode();
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[8];
    double N0;
    if (fread(hdr, 4, 8, f) != 8 || fread(&N0, 8, 1, f) != 1) return 3;
    const int M = hdr[0];
    const uint64_t N1 = (uint64_t)hdr[1];
    std::vector<uint64_t> rp(N1 + 1);
    if (fread(rp.data(), 8, N1 + 1, f) != N1 + 1) return 3;
    const uint64_t nnz = rp[N1];
    std::vector<int32_t> sid(nnz);
    std::vector<double> cp(nnz), ncp(N1), theta((size_t)M + 1);
    if (fread(sid.data(), 4, nnz, f) != nnz || fread(cp.data(), 8, nnz, f) != nnz || fread(ncp.data(), 8, N1, f) != N1 ||
        fread(theta.data(), 8, theta.size(), f) != theta.size()) return 3;
    fclose(f);
    if (M + 1 > kWindow) { fprintf(stderr, "estep_short_emu: every id must fit one window (M < %d)\n", kWindow); return 5; }
    HostLayout H;
    H.T = (uint32_t)hdr[2];
    uint64_t n_entries = 0;
    const uint64_t mask = build_layout_short(H, M, N1, rp.data(), sid.data(), cp.data(), ncp.data(), hdr[4] != 0, hdr[5], hdr[3], &n_entries);
    for (const Shape& S : H.shapes) printf("shape %d %d %d %d %u\n", S.fmt, S.lg, S.K, S.cut, S.n_rows);
    printf("entries %llu\nmask 0x%llx\n", (unsigned long long)n_entries, (unsigned long long)mask);
    {   // the planes read back: the CSR that went in (F64 shapes; Q32 planes hold rounded values)
        std::vector<int32_t> bsid(nnz, -1);
        std::vector<double> bcp(nnz, -1.0);
        bool same = true;
        for (const Shape& S : H.shapes) {
            if (S.fmt != kFmtF64) continue;
            for (uint32_t q = 0; q < S.n_rows; q++) {
                sell_unfill_row(S, H.T, S.row_base + q, H.order.data(), rp.data(), H.ssid.data(), H.sval.data(), bsid.data(), bcp.data());
                const uint32_t orig = H.order[S.row_base + q];
                for (uint64_t j = rp[orig]; j < rp[orig + 1]; j++) same = same && bsid[j] == sid[j] && !memcmp(&bcp[j], &cp[j], 8);
            }
        }
        printf("roundtrip %s\n", same ? "ok" : "BAD");
    }
    fflush(stdout);
    std::vector<double> counts((size_t)M + 1, 0.0);
    double tot_noise = 0.0, tot_neff = 0.0;
    Job* J = new Job();
    pthread_barrier_init(&J->blk.bar, nullptr, 256);
    for (int w = 0; w < 4; w++) pthread_barrier_init(&J->blk.w[w].bar, nullptr, 64);
    for (const Shape& S : H.shapes)
        for (uint32_t b0 = 0; b0 < S.n_slices; b0 += 4 * H.T) {
            J->H = &H;
            J->S = S;
            J->slice_begin = b0;
            J->n_slices = std::min<uint32_t>(4 * H.T, S.n_slices - b0);
            J->base = 0;
            J->span = M + 1;  // (every id inside: the loop without the global path, the one the headline runs)
            J->M = M;
            J->theta = theta.data();
            J->counts = counts.data();
            J->tot_noise = &tot_noise;
            J->tot_neff = &tot_neff;
            std::vector<std::thread> th;
            for (int t = 0; t < 256; t++) th.emplace_back(lane_body, J, t);
            for (auto& t : th) t.join();
        }
    delete J;
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    fwrite(counts.data(), 8, counts.size(), f);
    fwrite(&tot_noise, 8, 1, f);
    fwrite(&tot_neff, 8, 1, f);
    fclose(f);
    return 0;
}
