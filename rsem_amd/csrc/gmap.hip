// gmap.hip -- transcript coordinates -> genome coordinates and the per-read collapse on MI355X (rsem-tbam2gbam).
// Replaces, for every record of a transcript BAM, convert + tr2chr (BamConverter.h:150-191, sam_utils.h:137-208: a walk over the
// transcript's exons from the first one) and, for every read, CollapseMap (bc_aux.h: a std::map keyed by the converted alignments).
// The arithmetic is in gmap_block.hpp.
//
// A batch of whole groups (a group = the alignments of one read) goes through
//   k_gmap_count     a lane per mate: tid, pos, flag, n_cigar, bin and whether the CIGAR has an N;
//   hipcub::DeviceScan::ExclusiveSum     where every mate's CIGAR words start;
//   k_gmap_fill      a lane per mate: the words;
//   k_gmap_collapse  a wave per group of up to 64 alignments, a workgroup per longer one: the stable rank of every alignment inside
//                    its group, which alignments the map keeps, their weights folded in file order (float);
//   hipcub::DeviceScan::ExclusiveSum     the kept alignments' places in the output;
//   k_gmap_emit      (kept alignment, folded weight) pairs in output order.
// No atomics and no inline assembly: every result word has one writer.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <vector>

#include "gmap_block.hpp"
#include "stage_util.hpp"

using namespace rsem_gmapk;

namespace {

using rsem::blocks256;
using Buf = rsem::GrowBuf<4>;  // a device buffer that only grows

enum { B_TR, B_POS, B_LQ, B_FLAG, B_W, B_GOFF, B_SMALL, B_LARGE, B_OTID, B_OPOS, B_OFLAG, B_NCIG, B_BIN, B_HASN, B_COFF, B_CIGAR, B_ORDER, B_HEAD,
       B_WSUM, B_SCAN, B_OSRC, B_OW, B_TMP, B_COUNT };

}  // namespace

struct rsem_gmap {
    int device = 0;
    int32_t n_tr = 0;
    // the reference on the host (what the checks and the bounds need; uploaded when the first batch needs it)
    std::vector<uint8_t> minus;
    std::vector<int32_t> length, out_tid, start, end, cum;
    std::vector<uint64_t> exon_off;
    bool on_device = false;
    void *d_minus = nullptr, *d_length = nullptr, *d_out_tid = nullptr, *d_exon_off = nullptr, *d_start = nullptr, *d_end = nullptr, *d_cum = nullptr;
    rsem::StageQueue q;
    Buf buf[B_COUNT];
    size_t device_bytes = 0;
    std::mutex mu;  // one call at a time on a handle
};

namespace {

__global__ void __launch_bounds__(256) k_gmap_count(Ref R, uint32_t n_mates, const int32_t* __restrict__ tr, const int32_t* __restrict__ pos,
                                                     const int32_t* __restrict__ lq, const uint32_t* __restrict__ flag, int32_t* __restrict__ otid,
                                                     int32_t* __restrict__ opos, uint32_t* __restrict__ oflag, uint32_t* __restrict__ ncig,
                                                     uint32_t* __restrict__ bin, uint32_t* __restrict__ hasn) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n_mates) return;
    if (i == n_mates) { ncig[i] = 0u; return; }  // the scan's last output is the number of words
    const Mapped m = map_mate(R, tr[i], pos[i], lq[i], flag[i]);
    otid[i] = m.tid; opos[i] = m.pos; oflag[i] = m.flag; ncig[i] = m.n_cigar; bin[i] = m.bin; hasn[i] = m.has_n;
}

__global__ void __launch_bounds__(256) k_gmap_fill(Ref R, uint32_t n_mates, const int32_t* __restrict__ tr, const int32_t* __restrict__ pos,
                                                    const int32_t* __restrict__ lq, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ coff,
                                                    uint32_t* __restrict__ cigar) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_mates) return;
    const Mapped m = map_mate(R, tr[i], pos[i], lq[i], flag[i]);
    fill_cigar(R, tr[i], m, cigar + coff[i]);
}

// blocks [0, nb_small): four groups of up to 64 alignments each, a wave a group; the blocks behind them: one longer group each
__global__ void __launch_bounds__(kGroupThreads) k_gmap_collapse(uint32_t n_small, uint32_t nb_small, const uint32_t* __restrict__ small,
                                                                  const uint32_t* __restrict__ large, const uint32_t* __restrict__ goff, int mates,
                                                                  MateArrays A, const float* __restrict__ w, const uint32_t* __restrict__ cigar,
                                                                  uint32_t* __restrict__ order, uint32_t* __restrict__ head, float* __restrict__ wsum) {
    __shared__ Key stage[kGroupThreads];
    const int tid = RSEM_TIDX;
    if (blockIdx.x < nb_small) {
        const int wv = tid >> 6;
        const uint32_t idx = blockIdx.x * 4u + (uint32_t)wv;
        if (idx >= n_small) return;
        const uint32_t g = small[idx], g0 = goff[g];
        collapse_group<kWave>(g0, goff[g + 1] - g0, tid & 63, mates, A, w, cigar, stage + wv * kWave, order, head, wsum);
    } else {
        const uint32_t g = large[blockIdx.x - nb_small], g0 = goff[g];
        collapse_group<kGroupThreads>(g0, goff[g + 1] - g0, tid, mates, A, w, cigar, stage, order, head, wsum);
    }
}

__global__ void __launch_bounds__(256) k_gmap_emit(uint32_t n, const uint32_t* __restrict__ order, const uint32_t* __restrict__ head,
                                                    const float* __restrict__ wsum, const uint32_t* __restrict__ scan, uint32_t* __restrict__ osrc,
                                                    float* __restrict__ ow) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n || !head[p]) return;
    const uint32_t o = scan[p];
    osrc[o] = order[p];
    ow[o] = wsum[p];
}

int to_device(rsem_gmap* h) {
    RSEM_HIP_TRY(hipSetDevice(h->device));
    if (h->on_device) return RSEM_OK;
    RSEM_HIP_TRY(h->q.create());
    auto up = [&](void** d, const void* src, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(d, std::max<size_t>(bytes, 8));
        if (e != hipSuccess) return e;
        h->device_bytes += std::max<size_t>(bytes, 8);
        return bytes ? hipMemcpy(*d, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    RSEM_HIP_TRY(up(&h->d_minus, h->minus.data(), h->minus.size()));
    RSEM_HIP_TRY(up(&h->d_length, h->length.data(), h->length.size() * 4));
    RSEM_HIP_TRY(up(&h->d_out_tid, h->out_tid.data(), h->out_tid.size() * 4));
    RSEM_HIP_TRY(up(&h->d_exon_off, h->exon_off.data(), h->exon_off.size() * 8));
    RSEM_HIP_TRY(up(&h->d_start, h->start.data(), h->start.size() * 4));
    RSEM_HIP_TRY(up(&h->d_end, h->end.data(), h->end.size() * 4));
    RSEM_HIP_TRY(up(&h->d_cum, h->cum.data(), h->cum.size() * 4));
    h->on_device = true;
    return RSEM_OK;
}

struct Call {
    int mates;
    const uint64_t* group_off;
    const int32_t *tr, *pos, *l_qseq;
    const uint32_t* flag;
    const float* w;
    int32_t *out_tid, *out_pos;
    uint32_t *out_flag, *out_n_cigar, *out_bin, *out_has_n;
    uint64_t* cigar_off;
    uint32_t* cigar_words;
    uint64_t cigar_cap;
    uint64_t* out_src;
    float* out_w;
};

// the groups [glo, ghi) of the call: one batch.  words_done / out_done: CIGAR words and output alignments of the batches before.
int run_batch(rsem_gmap* h, const Call& c, uint64_t glo, uint64_t ghi, uint64_t& words_done, uint64_t& out_done, rsem_gmap_info* info,
              double& upload_ms, double& kernel_ms) {
    const uint64_t a_lo = c.group_off[glo], na64 = c.group_off[ghi] - a_lo, ng64 = ghi - glo;
    const uint32_t na = (uint32_t)na64, ng = (uint32_t)ng64, nm = na * (uint32_t)c.mates;
    const uint64_t m_lo = a_lo * (uint64_t)c.mates;
    // what the batch's CIGARs can take at most, the groups by size
    uint64_t bound = 0;
    for (uint32_t i = 0; i < nm; i++) { const int32_t t = c.tr[m_lo + i]; bound += 2 * (h->exon_off[t + 1] - h->exon_off[t]) + 2; }
    if (bound > 0xfffffff0ull) {
        rsem::set_last_error("rsem_gmap_convert: a batch whose CIGARs may take %llu words (2^32 at most: a smaller RSEM_GMAP_BATCH_ITEMS cuts it)", (unsigned long long)bound);
        return RSEM_ERR_INVALID;
    }
    std::vector<uint32_t> goff(ng + 1), small, large;
    for (uint32_t g = 0; g <= ng; g++) goff[g] = (uint32_t)(c.group_off[glo + g] - a_lo);
    for (uint32_t g = 0; g < ng; g++) (goff[g + 1] - goff[g] <= (uint32_t)kWave ? small : large).push_back(g);
    const uint32_t n_small = (uint32_t)small.size(), nb_small = (n_small + 3) / 4, n_large = (uint32_t)large.size();

    size_t t_scan_m = 0, t_scan_a = 0;
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan_m, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(nm + 1), h->q.st));
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan_a, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)(na + 1), h->q.st));
    const size_t tmp_bytes = std::max(t_scan_m, t_scan_a);
    const size_t need[B_COUNT] = {(size_t)nm * 4, (size_t)nm * 4, (size_t)nm * 4, (size_t)nm * 4, (size_t)na * 4, ((size_t)ng + 1) * 4, (size_t)ng * 4, (size_t)ng * 4,
                                  (size_t)nm * 4, (size_t)nm * 4, (size_t)nm * 4, ((size_t)nm + 1) * 4, (size_t)nm * 4, (size_t)nm * 4, ((size_t)nm + 1) * 4,
                                  (size_t)bound * 4, (size_t)na * 4, ((size_t)na + 1) * 4, (size_t)na * 4, ((size_t)na + 1) * 4, (size_t)na * 4, (size_t)na * 4, tmp_bytes};
    for (int b = 0; b < B_COUNT; b++) RSEM_HIP_TRY(h->buf[b].need(need[b], h->device_bytes));
    auto I32 = [&](int b) { return h->buf[b].as<int32_t>(); };
    auto U32 = [&](int b) { return h->buf[b].as<uint32_t>(); };
    auto F32 = [&](int b) { return h->buf[b].as<float>(); };
    hipStream_t st = h->q.st;
    const Ref R{(const uint8_t*)h->d_minus, (const int32_t*)h->d_length, (const int32_t*)h->d_out_tid, (const uint64_t*)h->d_exon_off,
                (const int32_t*)h->d_start, (const int32_t*)h->d_end, (const int32_t*)h->d_cum};

    RSEM_HIP_TRY(h->q.upload_begin());
    RSEM_HIP_TRY(hipMemcpyAsync(I32(B_TR), c.tr + m_lo, (size_t)nm * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(I32(B_POS), c.pos + m_lo, (size_t)nm * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(I32(B_LQ), c.l_qseq + m_lo, (size_t)nm * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(U32(B_FLAG), c.flag + m_lo, (size_t)nm * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(F32(B_W), c.w + a_lo, (size_t)na * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemcpyAsync(U32(B_GOFF), goff.data(), ((size_t)ng + 1) * 4, hipMemcpyHostToDevice, st));
    if (n_small) RSEM_HIP_TRY(hipMemcpyAsync(U32(B_SMALL), small.data(), (size_t)n_small * 4, hipMemcpyHostToDevice, st));
    if (n_large) RSEM_HIP_TRY(hipMemcpyAsync(U32(B_LARGE), large.data(), (size_t)n_large * 4, hipMemcpyHostToDevice, st));
    RSEM_HIP_TRY(hipMemsetAsync(U32(B_HEAD) + na, 0, 4, st));
    RSEM_HIP_TRY(h->q.upload_end());

    hipLaunchKernelGGL(k_gmap_count, dim3(blocks256((uint64_t)nm + 1)), dim3(256), 0, st, R, nm, I32(B_TR), I32(B_POS), I32(B_LQ), U32(B_FLAG), I32(B_OTID),
                       I32(B_OPOS), U32(B_OFLAG), U32(B_NCIG), U32(B_BIN), U32(B_HASN));
    size_t tb = h->buf[B_TMP].cap;
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(h->buf[B_TMP].p, tb, U32(B_NCIG), U32(B_COFF), (int)(nm + 1), st));
    // the words must fit what was allocated for them, and what the caller gave, before anything is written behind the offsets
    uint32_t words = 0;
    RSEM_HIP_TRY(hipMemcpyAsync(&words, U32(B_COFF) + nm, 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    if ((uint64_t)words > bound) {
        rsem::set_last_error("rsem_gmap_convert: %u CIGAR words on the device, %llu at most were expected", words, (unsigned long long)bound);
        return RSEM_ERR_STATE;
    }
    if (words_done + words > c.cigar_cap) {
        rsem::set_last_error("rsem_gmap_convert: the CIGARs take more than the %llu words of cigar_words", (unsigned long long)c.cigar_cap);
        return RSEM_ERR_INVALID;
    }
    hipLaunchKernelGGL(k_gmap_fill, dim3(blocks256(nm)), dim3(256), 0, st, R, nm, I32(B_TR), I32(B_POS), I32(B_LQ), U32(B_FLAG), U32(B_COFF), U32(B_CIGAR));
    const MateArrays A{I32(B_OTID), I32(B_OPOS), U32(B_OFLAG), U32(B_NCIG), U32(B_COFF)};
    hipLaunchKernelGGL(k_gmap_collapse, dim3(nb_small + n_large), dim3(kGroupThreads), 0, st, n_small, nb_small, U32(B_SMALL), U32(B_LARGE), U32(B_GOFF), c.mates, A,
                       F32(B_W), U32(B_CIGAR), U32(B_ORDER), U32(B_HEAD), F32(B_WSUM));
    tb = h->buf[B_TMP].cap;
    RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(h->buf[B_TMP].p, tb, U32(B_HEAD), U32(B_SCAN), (int)(na + 1), st));
    hipLaunchKernelGGL(k_gmap_emit, dim3(blocks256(na)), dim3(256), 0, st, na, U32(B_ORDER), U32(B_HEAD), F32(B_WSUM), U32(B_SCAN), U32(B_OSRC), F32(B_OW));
    RSEM_HIP_TRY(h->q.kernels_end());

    uint32_t n_out = 0;
    std::vector<uint32_t> coff(nm + 1), osrc(na);
    RSEM_HIP_TRY(hipMemcpyAsync(&n_out, U32(B_SCAN) + na, 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(c.out_tid + m_lo, I32(B_OTID), (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(c.out_pos + m_lo, I32(B_OPOS), (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(c.out_flag + m_lo, U32(B_OFLAG), (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(c.out_n_cigar + m_lo, U32(B_NCIG), (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(c.out_bin + m_lo, U32(B_BIN), (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(c.out_has_n + m_lo, U32(B_HASN), (size_t)nm * 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(coff.data(), U32(B_COFF), ((size_t)nm + 1) * 4, hipMemcpyDeviceToHost, st));
    if (words) RSEM_HIP_TRY(hipMemcpyAsync(c.cigar_words + words_done, U32(B_CIGAR), (size_t)words * 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(osrc.data(), U32(B_OSRC), (size_t)na * 4, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(c.out_w + out_done, F32(B_OW), (size_t)na * 4, hipMemcpyDeviceToHost, st));  // (n_out <= na of them count; out_done + na <= n_aln)
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    if (n_out < ng || n_out > na) {
        rsem::set_last_error("rsem_gmap_convert: %u alignments kept of %u in %u groups", n_out, na, ng);
        return RSEM_ERR_STATE;
    }
    for (uint32_t i = 0; i <= nm; i++) c.cigar_off[m_lo + i] = words_done + coff[i];
    for (uint32_t k = 0; k < n_out; k++) c.out_src[out_done + k] = a_lo + osrc[k];
    if (int rc = h->q.add_laps(upload_ms, kernel_ms)) return rc;
    words_done += words;
    out_done += n_out;
    if (info) info->n_launches += 6;
    return RSEM_OK;
}

}  // namespace

extern "C" int rsem_gmap_create(rsem_gmap** out, int device, int32_t n_transcripts, const uint8_t* strand, const int32_t* length, const int32_t* out_tid,
                                const uint64_t* exon_off, const int32_t* exon_start, const int32_t* exon_end) {
    RSEM_REQUIRE(out, "rsem_gmap_create: out must not be NULL");
    *out = nullptr;
    RSEM_REQUIRE(device >= 0, "rsem_gmap_create: device must not be negative");
    RSEM_REQUIRE(n_transcripts >= 0, "rsem_gmap_create: n_transcripts must not be negative");
    RSEM_REQUIRE(n_transcripts == 0 || (strand && length && out_tid && exon_off && exon_start && exon_end), "rsem_gmap_create: the transcript arrays must not be NULL");
    RSEM_REQUIRE(n_transcripts == 0 || exon_off[0] == 0, "rsem_gmap_create: exon_off must start at 0");
    for (int32_t t = 0; t < n_transcripts; t++) {
        if (strand[t] != '+' && strand[t] != '-') { rsem::set_last_error("rsem_gmap_create: transcript %d: strand must be '+' or '-'", t); return RSEM_ERR_INVALID; }
        if (out_tid[t] < 0) { rsem::set_last_error("rsem_gmap_create: transcript %d: negative output tid", t); return RSEM_ERR_INVALID; }
        if (exon_off[t + 1] <= exon_off[t] || exon_off[t + 1] - exon_off[t] > (uint64_t)kMaxExons) {
            rsem::set_last_error("rsem_gmap_create: transcript %d: 1 to %d exons are expected", t, kMaxExons);
            return RSEM_ERR_INVALID;
        }
        int64_t sum = 0;
        for (uint64_t e = exon_off[t]; e < exon_off[t + 1]; e++) {
            if (exon_start[e] < 1 || exon_end[e] < exon_start[e] || (e > exon_off[t] && exon_start[e] <= exon_end[e - 1])) {
                rsem::set_last_error("rsem_gmap_create: transcript %d: exons must be 1-based, of one base or more, ascending and apart", t);
                return RSEM_ERR_INVALID;
            }
            sum += (int64_t)exon_end[e] - exon_start[e] + 1;
        }
        if (sum != (int64_t)length[t]) {
            rsem::set_last_error("rsem_gmap_create: transcript %d: its exons have %lld bases, its length is %d", t, (long long)sum, length[t]);
            return RSEM_ERR_INVALID;
        }
    }
    rsem_gmap* h = new rsem_gmap();
    h->device = device;
    h->n_tr = n_transcripts;
    const uint64_t n_ex = n_transcripts ? exon_off[n_transcripts] : 0;
    h->minus.resize((size_t)n_transcripts);
    for (int32_t t = 0; t < n_transcripts; t++) h->minus[t] = strand[t] == '-';
    h->length.assign(length, length + n_transcripts);
    h->out_tid.assign(out_tid, out_tid + n_transcripts);
    if (n_transcripts) h->exon_off.assign(exon_off, exon_off + n_transcripts + 1); else h->exon_off.assign(1, 0);
    h->start.assign(exon_start, exon_start + n_ex);
    h->end.assign(exon_end, exon_end + n_ex);
    h->cum.resize((size_t)n_ex);
    for (int32_t t = 0; t < n_transcripts; t++) {
        int32_t c = 0;
        for (uint64_t e = exon_off[t]; e < exon_off[t + 1]; e++) { h->cum[e] = c; c += exon_end[e] - exon_start[e] + 1; }
    }
    *out = h;
    return RSEM_OK;
}

extern "C" void rsem_gmap_destroy(rsem_gmap* h) {
    if (!h) return;
    if (h->on_device) {
        (void)hipSetDevice(h->device);
        for (void* p : {h->d_minus, h->d_length, h->d_out_tid, h->d_exon_off, h->d_start, h->d_end, h->d_cum})
            if (p) (void)hipFree(p);
        for (Buf& b : h->buf) b.release(h->device_bytes);
        h->q.release();
    }
    delete h;
}

extern "C" int rsem_gmap_convert(rsem_gmap* h, int32_t mates, int64_t n_alignments, int64_t n_groups, const uint64_t* group_off, const int32_t* tr,
                                 const int32_t* pos, const int32_t* l_qseq, const uint32_t* flag, const float* w, int32_t* out_tid, int32_t* out_pos,
                                 uint32_t* out_flag, uint32_t* out_n_cigar, uint32_t* out_bin, uint32_t* out_has_n, uint64_t* cigar_off, uint32_t* cigar_words,
                                 uint64_t cigar_cap, uint64_t* out_src, float* out_w, rsem_gmap_info* info) {
    RSEM_REQUIRE(h, "rsem_gmap_convert: the handle must not be NULL");
    RSEM_REQUIRE(mates == 1 || mates == 2, "rsem_gmap_convert: mates must be 1 or 2");
    RSEM_REQUIRE(n_alignments >= 0 && n_groups >= 0, "rsem_gmap_convert: the counts must not be negative");
    RSEM_REQUIRE(n_alignments < (1ll << 40), "rsem_gmap_convert: 2^40 alignments or more in one call");
    RSEM_REQUIRE(group_off && cigar_off, "rsem_gmap_convert: group_off and cigar_off must not be NULL");
    RSEM_REQUIRE(n_alignments == 0 || (tr && pos && l_qseq && flag && w && out_tid && out_pos && out_flag && out_n_cigar && out_bin && out_has_n && out_src && out_w),
                 "rsem_gmap_convert: the per-mate and per-alignment arrays must not be NULL");
    RSEM_REQUIRE(cigar_cap == 0 || cigar_words, "rsem_gmap_convert: cigar_words must not be NULL");
    RSEM_REQUIRE(group_off[0] == 0 && group_off[n_groups] == (uint64_t)n_alignments, "rsem_gmap_convert: group_off must start at 0 and end at n_alignments");
    for (int64_t g = 0; g < n_groups; g++)
        if (group_off[g + 1] <= group_off[g]) { rsem::set_last_error("rsem_gmap_convert: group_off does not ascend at group %lld", (long long)g); return RSEM_ERR_INVALID; }
    const uint64_t n_mates = (uint64_t)n_alignments * (uint64_t)mates;
    for (uint64_t i = 0; i < n_mates; i++) {
        if (tr[i] < 0 || tr[i] >= h->n_tr) { rsem::set_last_error("rsem_gmap_convert: mate %llu: transcript index %d of %d", (unsigned long long)i, tr[i], h->n_tr); return RSEM_ERR_INVALID; }
        if (pos[i] < 0 || l_qseq[i] < 1 || (int64_t)pos[i] + l_qseq[i] > 0x7fffffffll) {
            rsem::set_last_error("rsem_gmap_convert: mate %llu: position %d, %d bases", (unsigned long long)i, pos[i], l_qseq[i]);
            return RSEM_ERR_INVALID;
        }
    }
    uint64_t budget = kDefaultBatchItems;
    if (int rc = rsem::env_whole("RSEM_GMAP_BATCH_ITEMS", 1, LLONG_MAX, &budget)) return rc;  // a test and measurement knob, read at call time
    if (info) {
        memset(info, 0, sizeof(*info));
        info->batch_items = budget;
        info->n_groups = (uint64_t)n_groups;
        info->n_alignments_in = (uint64_t)n_alignments;
    }
    cigar_off[0] = 0;
    if (n_alignments == 0) return RSEM_OK;  // nothing to convert: no device needed
    std::vector<std::pair<uint64_t, uint64_t>> batches;
    for (uint64_t lo = 0; lo < (uint64_t)n_groups;) {
        const uint64_t hi = batch_end(group_off, (uint64_t)n_groups, lo, budget);
        if (group_off[hi] - group_off[lo] > 0x3fffffffull) {
            rsem::set_last_error("rsem_gmap_convert: a batch of %llu alignments (2^30 - 1 at most)", (unsigned long long)(group_off[hi] - group_off[lo]));
            return RSEM_ERR_INVALID;
        }
        batches.push_back({lo, hi});
        lo = hi;
    }
    std::lock_guard<std::mutex> lock(h->mu);
    if (int rc = to_device(h)) return rc;
    const Call c{mates, group_off, tr, pos, l_qseq, flag, w, out_tid, out_pos, out_flag, out_n_cigar, out_bin, out_has_n, cigar_off, cigar_words, cigar_cap, out_src, out_w};
    uint64_t words_done = 0, out_done = 0;
    double upload_ms = 0, kernel_ms = 0;
    for (const auto& b : batches)
        if (int rc = run_batch(h, c, b.first, b.second, words_done, out_done, info, upload_ms, kernel_ms)) return rc;
    if (info) {
        info->n_alignments_out = out_done;
        info->n_cigar_words = words_done;
        info->n_batches = (int32_t)batches.size();
        info->device_bytes = h->device_bytes;
        info->upload_ms = upload_ms;
        info->kernel_ms = kernel_ms;
    }
    return RSEM_OK;
}
