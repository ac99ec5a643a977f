// estep_start_emu.cpp -- TEST INFRASTRUCTURE: the start list of the sliced layout (sell_layout.hpp: start_list_count /
// start_list_fill_lane -- per marked slice the ids of the lanes that start a tuple, K * popcount(mask) entries, and the exclusive
// sums that say where they begin) on the CPU, and the kernel body (estep_block.hpp, one OS thread per lane as in tests/estep_emu.cpp)
// reading a new tuple's ids from that list instead of the id planes.
//
//   estep_start_emu in.bin out.bin
//       in:  i32 M, N1, T, min_units (short classes: 0 off, -1 every class, > 0 the threshold), q32 (0/1), range_bits, from_counts (0/1),
//                window (0: 2048; smaller: forces ids outside a unit's window, and is the reach of the sort key's apart bit),
//                policy (0: whole rows; 2: reads mostly outside their window split; 3: every read with an id outside splits),
//                use_list (0: every marked slice reads its id planes; 1: the start list), quarter (1: quarter-size units, one block each,
//                a wave begins in the middle of a block), far_queue (1: units with ids outside take the far-queue loop; 0: the loop
//                with global atomics, which takes the list), run (0: build and check the list only); 3 x i32 pad; f64 N0
//            u64 row_ptr[N1+1]; i32 sid[nnz]; f64 cp[nnz]; f64 ncp[N1]; f64 theta[M+1] (from_counts: counts[M+1] + 2 * 64 totals)
//       out: f64 counts[M+1], f64 noise total, f64 reads with a non-zero normaliser
//       stdout: "slices N", "marked N", "entries N", "maxn N" (the most starting lanes in one slice), "list ok" or lines starting "BAD";
//               "traffic FIRST ENTRIES SLICES MARKED" and "traffic ok": sid_traffic_of_wave (what rsem_em_get_info's byte accounting sums
//               over the unit table) against a count made slice by slice from the masks
// Build (tests/test_estep_start_list_cpu.py): hipcc -DRSEM_EMU [-DRSEM_F64_DEPTHS=3,3,3,3 -DRSEM_Q32_DEPTHS=3,3,3,3] tests/estep_start_emu.cpp -lpthread
#include "simt_emu.hpp"

namespace {
using rsem::kEpsilon;
constexpr int kTotSlots = 64;
constexpr int kWindow = 2048;
#include "../rsem_amd/csrc/estep_block.hpp"
}  // namespace

// the layout: row_key_of with short classes, apart bit and split rows; shapes by shape_of_id; planes by sell_fill_row; masks by
// slice_lane_changed / read_lanes_of (the bodies of the construction kernels)
static void build_layout_all(HostLayout& H, int M, uint64_t N1, const uint64_t* rp, const int32_t* sid, const double* cp, const double* ncp, int policy,
                             bool q32, int range_bits, int apart, int min_units) {
    unsigned long long hist[2 * kLenHist] = {};
    for (uint64_t i = 0; i < N1; i++) {
        const uint64_t fr = rp[i], to = rp[i + 1];
        if (to - fr > 256) continue;
        const int fmt = (q32 && row_takes_q32(cp, fr, to, range_bits)) ? kFmtQ32 : kFmtF64;
        hist[fmt * kLenHist + (to - fr)]++;
    }
    const uint64_t classes = min_units > 0 ? short_classes_worth_it(hist, 1, H.T, min_units) : (min_units < 0 ? ~0ull : 0ull);
    std::vector<std::pair<uint64_t, uint32_t>> keyed(N1);
    for (uint64_t i = 0; i < N1; i++) {
        int err = 0;
        const uint64_t key = row_key_of(i, M, rp, sid, q32 ? cp : nullptr, range_bits, apart, &err, policy == 2 ? 1 : (policy == 3 ? 2 : 0), nullptr, classes);
        if (err || (int)(key >> (64 - kShapeBits)) == kLongShape) { fprintf(stderr, "estep_start_emu: bad CSR / long row\n"); exit(2); }
        keyed[i] = {key, (uint32_t)i};
    }
    std::stable_sort(keyed.begin(), keyed.end());
    H.order.resize(N1);
    for (uint64_t p = 0; p < N1; p++) H.order[p] = keyed[p].second;
    uint64_t n_planes = 0, val_bytes = 0;
    uint32_t n_slots = 0;
    for (uint64_t p = 0; p < N1;) {
        const int id = (int)(keyed[p].first >> (64 - kShapeBits));
        uint64_t e = p;
        while (e < N1 && (int)(keyed[e].first >> (64 - kShapeBits)) == id) ++e;
        Shape S{};
        int fmt, lg, K, cut;
        if (!shape_of_id(id, fmt, lg, K, cut)) { fprintf(stderr, "estep_start_emu: shape id %d\n", id); exit(2); }
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
        if (S.fmt == kFmtF64X && !H.has_x) { H.x_slot_base = n_slots; H.has_x = true; }
        n_slots += S.n_slices * rps;
        val_bytes += shape_val_bytes(S);
        H.shapes.push_back(S);
        p = e;
    }
    H.ssid.assign(n_planes * 64, 0);
    H.sval.assign(val_bytes + 8, 0);
    H.sncp.assign(n_slots + 1, 0.0);
    H.sexp.assign(n_slots + 1, 0);
    H.n_slots = n_slots;
    if (!H.has_x) H.x_slot_base = n_slots;
    for (const Shape& S : H.shapes)
        for (uint32_t q = 0; q < S.n_rows; q++) {
            int err = 0;
            const uint32_t anchor = (uint32_t)((keyed[S.row_base + q].first >> 32) & kKeyMinSidCap);
            sell_fill_row<true>(S, H.T, S.row_base + q, H.order.data(), rp, sid, cp, ncp, H.ssid.data(), H.sval.data(), H.sncp.data(), H.sexp.data(), &err,
                                anchor, apart);
            if (err) { fprintf(stderr, "estep_start_emu: sell_fill_row error %d\n", err); exit(2); }
            if (S.fmt == kFmtF64X) {
                uint32_t sl, r;
                row_to_slot(S, H.T, q, sl, r);
                const uint32_t slot = S.slot_base + sl * shape_R(S) + r;
                const uint32_t orig = H.order[S.row_base + q];
                for (uint64_t j = rp[orig]; j < rp[orig + 1]; j++)
                    if (!in_split_window(sid[j], anchor, apart)) H.far.push_back({sid[j], cp ? cp[j] : 0.0, slot});
            }
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
}

// the list, by the product's own functions (the bodies of k_start_counts / the scan / k_start_fill) ...
static void build_start_list(const HostLayout& H, std::vector<uint32_t>& off, std::vector<int32_t>& list) {
    off.assign(H.n_slices, 0);
    uint64_t total = 0;
    for (const Shape& S : H.shapes)
        for (uint32_t sl = 0; sl < S.n_slices; sl++) {
            off[S.slice_base + sl] = (uint32_t)total;
            total += start_list_count(S.K, H.masks[S.slice_base + sl]);
        }
    list.assign(total + kStartListPad, -1);
    for (const Shape& S : H.shapes)
        for (uint32_t sl = 0; sl < S.n_slices; sl++)
            for (int lane = 0; lane < 64; lane++)
                start_list_fill_lane(S, sl, lane, H.masks[S.slice_base + sl], off[S.slice_base + sl], H.ssid.data(), list.data());
}
// ... and what it must hold, spelled out bit by bit
static int check_start_list(const HostLayout& H, const std::vector<uint32_t>& off, const std::vector<int32_t>& list) {
    int bad = 0;
    uint64_t at = 0, marked = 0;
    int maxn = 0;
    for (const Shape& S : H.shapes)
        for (uint32_t sl = 0; sl < S.n_slices; sl++) {
            const uint32_t s = S.slice_base + sl;
            const unsigned long long m = H.masks[s];
            if (off[s] != at) { if (bad++ < 10) printf("BAD offset of slice %u: %u, expected %llu\n", s, off[s], (unsigned long long)at); }
            int n = 0;
            for (int l = 0; l < 64; l++) n += (int)((m >> l) & 1ull);
            maxn = std::max(maxn, n);
            marked += n != 0;
            for (int k = 0; k < S.K; k++) {
                int rank = 0;
                for (int l = 0; l < 64; l++) {
                    if (((m >> l) & 1ull) == 0ull) continue;
                    const int32_t want = H.ssid[(S.plane_base + (uint64_t)sl * S.K + k) * 64 + l];
                    const int32_t got = list[at + (uint64_t)k * n + rank];
                    if (got != want) { if (bad++ < 10) printf("BAD slice %u plane %d lane %d: list %d, plane %d\n", s, k, l, got, want); }
                    ++rank;
                }
            }
            at += (uint64_t)S.K * n;
        }
    if (at + kStartListPad != list.size()) { printf("BAD total %llu entries, list of %zu\n", (unsigned long long)at, list.size()); ++bad; }
    for (uint64_t i = at; i < list.size(); i++)
        if (list[i] != -1) { printf("BAD entry %llu behind the end was written\n", (unsigned long long)i); ++bad; break; }
    printf("slices %u\nmarked %llu\nentries %llu\nmaxn %d\n", H.n_slices, (unsigned long long)marked, (unsigned long long)at, maxn);
    if (!bad) printf("list ok\n");
    return bad;
}

// the units as sell_build_units cuts them: four blocks, a block per wave -- or (quarter) one block, a quarter of it per wave; windows and
// the far flag by the rule of sell_flag_far_units
static std::vector<Unit> cut_units(const HostLayout& H, bool quarter, int window) {
    std::vector<Unit> units;
    const uint32_t unit_slices = quarter ? H.T : 4 * H.T, per_wave = quarter ? (H.T + 3) / 4 : H.T;
    for (size_t sh = 0; sh < H.shapes.size(); sh++) {
        const Shape& S = H.shapes[sh];
        for (uint32_t b0 = 0; b0 < S.n_slices; b0 += unit_slices) {
            Unit U{};
            U.shape = (int32_t)sh;
            U.S = S;
            U.slice_begin = b0;
            U.n_slices = std::min<uint32_t>(unit_slices, S.n_slices - b0);
            U.per_wave = per_wave;
            int lo = 0x7fffffff, hi = 0;
            const uint64_t p0 = (S.plane_base + (uint64_t)b0 * S.K) * 64, p1 = (S.plane_base + (uint64_t)(b0 + U.n_slices) * S.K) * 64;
            for (uint64_t p = p0; p < p1; p++)
                if (H.ssid[p] > 0) { lo = std::min(lo, (int)H.ssid[p]); hi = std::max(hi, (int)H.ssid[p]); }
            if (lo > hi) { lo = 1; hi = 1; }
            U.base = lo;
            U.span = std::min(hi - lo + 1, window);
            for (uint64_t p = p0; p < p1; p++) U.pad[0] = U.pad[0] || unit_entry_is_far(U, H.ssid[p]);
            units.push_back(U);
        }
    }
    return units;
}

// The byte accounting's rule (sid_traffic_of_wave, summed over the units' four waves) against a count that walks the SLICES: a slice is
// a wave's first slice, or a later one, or belongs to a unit of the far-queue launch -- marked here in an array of its own.
static int check_traffic(const HostLayout& H, const std::vector<Unit>& units, bool far_queue) {
    SidTraffic got;
    std::vector<int> kind(H.n_slices, -1);  // 0: first slice of a wave, 1: a later slice, 2: far-queue unit
    for (const Unit& U : units) {
        const bool fq = far_queue && U.pad[0] != 0 && U.S.fmt != kFmtF64X;  // (the dispatch of lane_body below)
        for (uint32_t w = 0; w < 4; w++) {
            const SidTraffic t = sid_traffic_of_wave(U, w, fq, H.masks.data());
            got.first_planes += t.first_planes; got.list_entries += t.list_entries; got.list_slices += t.list_slices; got.marked_planes += t.marked_planes;
        }
        const uint32_t s0 = U.S.slice_base + U.slice_begin;
        for (uint32_t i = 0; i < U.n_slices; i++) {
            if (kind[s0 + i] != -1) { printf("BAD slice %u belongs to two units\n", s0 + i); return 1; }
            kind[s0 + i] = fq ? 2 : (i % U.per_wave == 0 ? 0 : 1);
        }
        if (U.n_slices > 4 * U.per_wave) { printf("BAD unit of %u slices, %u per wave\n", U.n_slices, U.per_wave); return 1; }
    }
    SidTraffic want;
    for (const Shape& S : H.shapes)
        for (uint32_t sl = 0; sl < S.n_slices; sl++) {
            const uint32_t s = S.slice_base + sl;
            int n = 0;
            for (int l = 0; l < 64; l++) n += (int)((H.masks[s] >> l) & 1ull);
            if (kind[s] == -1) { printf("BAD slice %u belongs to no unit\n", s); return 1; }
            if (kind[s] == 2) want.marked_planes += n ? S.K : 0;
            else {
                want.list_slices += 1;
                if (kind[s] == 0) want.first_planes += S.K;
                else want.list_entries += (unsigned long long)S.K * n;
            }
        }
    printf("traffic %llu %llu %llu %llu\n", got.first_planes, got.list_entries, got.list_slices, got.marked_planes);
    if (got.first_planes != want.first_planes || got.list_entries != want.list_entries || got.list_slices != want.list_slices || got.marked_planes != want.marked_planes) {
        printf("BAD traffic: slice by slice %llu %llu %llu %llu\n", want.first_planes, want.list_entries, want.list_slices, want.marked_planes);
        return 1;
    }
    printf("traffic ok\n");
    return 0;
}

struct Job {
    const HostLayout* H;
    Shape S;
    uint32_t slice_begin, n_slices, per_wave;
    int base, span, M;
    bool far, far_queue;
    const double* theta;
    double N0;
    double* counts;
    double* tot_noise;
    double* tot_neff;
    double th_win[kWindow], cnt_win[kWindow];
    XArgs xa;
    StartList sl;
    int fq_sid[4][kFarQCap];
    double fq_val[4][kFarQCap];
    int fq_n[4];
    emu::Block blk;
};

template <bool kFC>
static void lane_body(Job* J, int tid) {
    emu::t_tid = tid;
    emu::t_blk = &J->blk;
    const int lane = tid & 63, w = tid >> 6;
    const HostLayout& H = *J->H;
    const Shape& S = J->S;
    const uint32_t u_end = S.slice_base + J->slice_begin + J->n_slices;
    const uint32_t s_begin = S.slice_base + J->slice_begin + (uint32_t)w * J->per_wave;
    const uint32_t s_end = std::min(u_end, s_begin + J->per_wave);
    const double* tsrc = J->theta + J->M + 1;
    double noise = 0.0, neff = 0.0;
    FarQueue fq;
    fq.sid = J->fq_sid[w]; fq.val = J->fq_val[w]; fq.n = &J->fq_n[w];
    if (lane == 0) J->fq_n[w] = 0;
    // the dispatch of k_estep_lane (em.hip): the launches without far queue are handed the list, the far-queue launch is not
#define EMU_BLOCK(KK, QQ, FF, XX)                                                                                                      \
    estep_block<KK, kFC, QQ, (QQ ? kQ32Depth[KK - 1] : kF64Depth[KK - 1]), FF, XX>(S, s_begin, s_end, lane, J->base, J->span, J->theta, tsrc, J->N0, \
        J->th_win, J->cnt_win, H.sval.data(), H.sexp.data(), H.ssid.data(), H.sncp.data(), H.masks.data(), J->counts, noise, neff, J->M, J->xa, FarQueue(), J->sl)
#define EMU_BLOCK_FQ(KK, QQ)                                                                                                          \
    estep_block<KK, kFC, QQ, 3, true, false, true>(S, s_begin, s_end, lane, J->base, J->span, J->theta, tsrc, J->N0, \
        J->th_win, J->cnt_win, H.sval.data(), H.sexp.data(), H.ssid.data(), H.sncp.data(), H.masks.data(), J->counts, noise, neff, J->M, J->xa, fq)
    const int code = (S.K - 1) | ((S.fmt == kFmtQ32 ? 1 : 0) << 2) | ((J->far ? 1 : 0) << 3) | (((!kFC && S.fmt == kFmtF64X) ? 1 : 0) << 4);
    if (s_begin < u_end) switch (code) {
        case 0: EMU_BLOCK(1, false, false, false); break;
        case 1: EMU_BLOCK(2, false, false, false); break;
        case 2: EMU_BLOCK(3, false, false, false); break;
        case 3: EMU_BLOCK(4, false, false, false); break;
        case 4: EMU_BLOCK(1, true, false, false); break;
        case 5: EMU_BLOCK(2, true, false, false); break;
        case 6: EMU_BLOCK(3, true, false, false); break;
        case 7: EMU_BLOCK(4, true, false, false); break;
        case 8: if (J->far_queue) EMU_BLOCK_FQ(1, false); else EMU_BLOCK(1, false, true, false); break;
        case 9: if (J->far_queue) EMU_BLOCK_FQ(2, false); else EMU_BLOCK(2, false, true, false); break;
        case 10: if (J->far_queue) EMU_BLOCK_FQ(3, false); else EMU_BLOCK(3, false, true, false); break;
        case 11: if (J->far_queue) EMU_BLOCK_FQ(4, false); else EMU_BLOCK(4, false, true, false); break;
        case 12: if (J->far_queue) EMU_BLOCK_FQ(1, true); else EMU_BLOCK(1, true, true, false); break;
        case 13: if (J->far_queue) EMU_BLOCK_FQ(2, true); else EMU_BLOCK(2, true, true, false); break;
        case 14: if (J->far_queue) EMU_BLOCK_FQ(3, true); else EMU_BLOCK(3, true, true, false); break;
        case 15: if (J->far_queue) EMU_BLOCK_FQ(4, true); else EMU_BLOCK(4, true, true, false); break;
        default:
            if constexpr (!kFC) switch (code & 11) {
                case 0: EMU_BLOCK(1, false, false, true); break;
                case 1: EMU_BLOCK(2, false, false, true); break;
                case 2: EMU_BLOCK(3, false, false, true); break;
                case 3: EMU_BLOCK(4, false, false, true); break;
                case 8: EMU_BLOCK(1, false, true, true); break;
                case 9: EMU_BLOCK(2, false, true, true); break;
                case 10: EMU_BLOCK(3, false, true, true); break;
                default: EMU_BLOCK(4, false, true, true); break;
            }
            break;
    } else {
        const ThetaSrc th = theta_src<kFC>(J->theta, tsrc, J->N0, lane);
        stage_windows<kFC>(J->base, J->span, J->M, th, J->th_win, J->cnt_win);
    }
#undef EMU_BLOCK
#undef EMU_BLOCK_FQ
    RSEM_SYNC();
    for (int i = tid; i < J->span; i += 256)
        if (J->cnt_win[i] != 0.0) emu::atomic_add(&J->counts[J->base + i], J->cnt_win[i]);
    emu::atomic_add(J->tot_noise, noise);
    emu::atomic_add(J->tot_neff, neff);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t hdr[16];
    double N0;
    if (fread(hdr, 4, 16, f) != 16 || fread(&N0, 8, 1, f) != 1) return 3;
    const int M = hdr[0];
    const uint64_t N1 = (uint64_t)hdr[1];
    const int min_units = hdr[3], range_bits = hdr[5], window = hdr[7] > 0 ? hdr[7] : kWindow, policy = hdr[8];
    const bool q32 = hdr[4] != 0, from_counts = hdr[6] != 0, use_list = hdr[9] != 0, quarter = hdr[10] != 0, far_queue = hdr[11] != 0, run = hdr[12] != 0;
    std::vector<uint64_t> rp(N1 + 1);
    if (fread(rp.data(), 8, N1 + 1, f) != N1 + 1) return 3;
    const uint64_t nnz = rp[N1];
    std::vector<int32_t> sid(nnz);
    std::vector<double> cp(nnz), ncp(N1);
    std::vector<double> theta((size_t)M + 1 + (from_counts ? 2 * kTotSlots : 0));
    if (fread(sid.data(), 4, nnz, f) != nnz || fread(cp.data(), 8, nnz, f) != nnz || fread(ncp.data(), 8, N1, f) != N1 ||
        fread(theta.data(), 8, theta.size(), f) != theta.size()) return 3;
    fclose(f);
    HostLayout H;
    H.T = (uint32_t)hdr[2];
    build_layout_all(H, M, N1, rp.data(), sid.data(), cp.data(), ncp.data(), policy, q32, range_bits, hdr[7] > 0 ? hdr[7] : kLayoutWindow, min_units);
    std::vector<uint32_t> start_off;
    std::vector<int32_t> start_list;
    build_start_list(H, start_off, start_list);
    const std::vector<Unit> units = cut_units(H, quarter, window);
    const int bad = check_start_list(H, start_off, start_list) + check_traffic(H, units, far_queue);
    fflush(stdout);
    if (bad) return 6;
    if (!run) return 0;
    std::vector<double> counts((size_t)M + 1, 0.0);
    double tot_noise = 0.0, tot_neff = 0.0;
    std::vector<double> xextra(H.n_slots - H.x_slot_base + 1, 0.0), xinv(H.n_slots - H.x_slot_base + 1, 0.0);
    if (!H.far.empty() && from_counts) { fprintf(stderr, "estep_start_emu: split rows need a plain theta\n"); return 5; }
    for (const HostLayout::Far& e : H.far) {  // k_far_rowsum
        double fv = theta[e.sid] * e.cp;
        if (fv < kEpsilon) fv = 0.0;
        xextra[e.slot - H.x_slot_base] += fv;
    }
    Job* J = new Job();
    J->far_queue = far_queue;
    J->xa.extra = xextra.data();
    J->xa.inv = xinv.data();
    J->xa.slot_base = H.x_slot_base;
    if (use_list) { J->sl.list = start_list.data(); J->sl.off = start_off.data(); }
    pthread_barrier_init(&J->blk.bar, nullptr, 256);
    for (int w = 0; w < 4; w++) pthread_barrier_init(&J->blk.w[w].bar, nullptr, 64);
    for (const Unit& U : units) {
        {
            J->H = &H;
            J->S = U.S;
            J->slice_begin = U.slice_begin;
            J->n_slices = U.n_slices;
            J->per_wave = U.per_wave;
            J->base = U.base;
            J->span = U.span;
            J->far = U.pad[0] != 0;
            J->M = M;
            J->theta = theta.data();
            J->N0 = N0;
            J->counts = counts.data();
            J->tot_noise = &tot_noise;
            J->tot_neff = &tot_neff;
            std::vector<std::thread> th;
            for (int t = 0; t < 256; t++) th.emplace_back(from_counts ? lane_body<true> : lane_body<false>, J, t);
            for (auto& t : th) t.join();
        }
    }
    for (const HostLayout::Far& e : H.far) {  // k_far_colsum
        double fv = theta[e.sid] * e.cp;
        if (fv < kEpsilon) fv = 0.0;
        counts[e.sid] += fv * xinv[e.slot - H.x_slot_base];
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
