// model.hip -- RSEM's read models on MI355X: P(read, alignment | transcript) for every alignment
// (rounds 1-11 of rsem-run-em) and the posterior-weighted sufficient statistics that re-estimate
// the model in rounds 1-10.  C ABI: include/rsem_hip.h (rsem_model_*).
//
// Reference semantics restated here (file:line under /root/reference):
//   getConPrb       SingleModel.h:95-146, SingleQModel.h:101-151, PairedEndModel.h:90-134, PairedEndQModel.h:94-138
//   getNoiseConPrb  SingleQModel.h:153-162, PairedEndQModel.h:140-155 (and twins)
//   update          SingleQModel.h:168-215, PairedEndQModel.h:161-180;  updateNoise :217-221 / :182-188
//   parts           LenDist.h:56-77, RSPD.h:43-75, QProfile.h:88-120, Profile.h:91-120,
//                   NoiseQProfile.h:74-114, NoiseProfile.h:64-101, RefSeq.h:84-92
// The reference re-reads every read from FASTA/FASTQ text each round (EM.cpp:200-202); here reads and
// transcript sequences are uploaded once as byte codes and stay in HBM.
//   k_conprb : one thread per alignment (product over the read's bases of table entries).
//   k_noise  : one thread per read.
//   k_update : one thread per alignment; weighted histograms accumulate in per-workgroup LDS tables
//              (ds_add_f64) and are merged with one device atomic per touched entry.
#include <cmath>
#include <thread>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "em_internal.hpp"
#include "upload.hpp"

namespace {

using rsem::kEpsilon;
constexpr int kBlk = 256;

// tables, data views, the scalar pieces of getConPrb / update, and the group-per-read body of the model rounds' kernel
#include "sell_shape.hpp"
#include "model_block.hpp"

// Do two strand windows of `len` bases hold the same bases?  The alignments of a read mostly do: isoforms of a gene share
// the exon the read came from, which is WHY the read is multi-mapped.  Then the profile product of the read against the
// window (the expensive part of getConPrb) and the profile counts it feeds (update) are the same for both alignments.
__device__ inline bool same_window(const uint64_t* __restrict__ refw, uint64_t a, uint64_t b, int len) {
    if (a == b) return true;
    const uint64_t* ra = refw + (a >> 3);
    const uint64_t* rb = refw + (b >> 3);
    const int sa = (int)(a & 7) * 8, sb = (int)(b & 7) * 8;
    uint64_t a0 = ra[0], b0 = rb[0];
    for (int i = 0; i < len; i += 8) {
        const uint64_t a1 = ra[(i >> 3) + 1], b1 = rb[(i >> 3) + 1];
        uint64_t x = funnel8(a0, a1, sa) ^ funnel8(b0, b1, sb);
        a0 = a1; b0 = b1;
        const int n = len - i;
        if (n < 8) x &= (1ull << (8 * n)) - 1ull;
        if (x) return false;
    }
    return true;
}

// same_prev flags (DevData): one thread per alignment, once per model context
template <bool kPE>
__global__ __launch_bounds__(kBlk) void k_window_flags(DevData D, uint8_t* flags) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= D.nnz) return;
    const uint32_t row = D.hit_row[j];
    uint8_t f = 0;
    // low-quality reads are never walked (and their coordinates were not range-checked); a read's first alignment has no predecessor
    if (!D.lq[row] && j > D.row_ptr[row]) {
        auto windows = [&](uint64_t k, uint64_t& a1, uint64_t& a2) {
            const int s = D.sid_signed[k];
            const int sid = s < 0 ? -s : s, dir = s < 0 ? 1 : 0;
            const int pos = D.pos[k];
            a1 = D.soff[2 * sid + dir] + pos;
            a2 = kPE ? D.soff[2 * sid + (!dir)] + (D.totLen[sid] - pos - D.insertL[k]) : 0;
        };
        uint64_t a1, a2, p1, p2;
        windows(j, a1, a2);
        windows(j - 1, p1, p2);
        if (same_window(D.refw, a1, p1, D.rlen[0][row])) f |= 1;
        if (kPE && same_window(D.refw, a2, p2, D.rlen[1][row])) f |= 2;
    }
    flags[j] = f;
}

// DevData::aw0 .. atot and bit 2 of the flags (model_block.hpp alignment_fields): one thread per alignment, once per model context
// and seed length.  Low-quality reads are never walked (and their coordinates were not range-checked): zeros.
// kWide: + the addresses' bits 32..39 (aw0h / aw1h; not touched otherwise).
template <bool kPE, bool kWide = false>
__global__ __launch_bounds__(kBlk) void k_alignment_fields(DevData D, int seedLen, uint32_t* aw0, uint32_t* aw1, uint32_t* afull, uint32_t* atot, uint8_t* flags,
                                                           uint8_t* aw0h = nullptr, uint8_t* aw1h = nullptr) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= D.nnz) return;
    AlnFields F{0u, 0u, 1u, 1u, false};
    if (!D.lq[D.hit_row[j]]) F = alignment_fields<kPE, kWide>(D, seedLen, j);
    aw0[j] = F.a0;
    if (kPE) aw1[j] = F.a1;
    if (kWide) aw0h[j] = F.h0;
    if (kWide && kPE) aw1h[j] = F.h1;
    afull[j] = F.full;
    atot[j] = F.tot;
    flags[j] = (uint8_t)((flags[j] & 3u) | (F.masked ? 4u : 0u));
}

// The model rounds' kernel (model_block.hpp): a group of 16 lanes per read, 512 threads per workgroup (two per CU: the
// probability and count tables take 57 KB of LDS each), persistent grid, reads dealt to the waves four at a time.
constexpr int kGroupBlk = 512;
#ifndef RSEM_GROUP_CHUNK
#define RSEM_GROUP_CHUNK 256
#endif
constexpr int kGroupChunk = RSEM_GROUP_CHUNK;  // rows per chunk (a multiple of the 32 rows a workgroup takes per step)
// (a workgroup's last step in a chunk is not cut at the chunk's end: with any other value the rows behind it are counted twice)
static_assert(kGroupBlk / 64 * 4 == 32 && (kGroupChunk == 0 || (kGroupChunk > 0 && kGroupChunk % 32 == 0)),
              "RSEM_GROUP_CHUNK: 0 or a multiple of the 32 rows a workgroup takes per step");
// 4 waves per SIMD (<= 128 VGPRs, a few dwords of scratch in the variants with the update) instead of the 2-3 the
// allocator would settle for: 14.1 against 17.1 ms per round at a fifth of configs[2] (profiles/r04b_call.log) -- the kernel
// waits on dependent loads, and the fourth wave hides more of them than the spills cost.
#ifndef RSEM_GROUP_ATTR
#define RSEM_GROUP_ATTR __attribute__((amdgpu_waves_per_eu(4, 4)))
#endif
template <bool kQ, bool kPE, bool kUpdate, bool kWide = false>
__global__ __launch_bounds__(kGroupBlk) RSEM_GROUP_ATTR void k_model_group(DevData D, DevTables T, const double* __restrict__ theta, double* __restrict__ cp,
                                                             double* __restrict__ ncp, AccumPtrs A, PlaneOut PO) {
    __shared__ double s_prob[kQ ? kQProbLds : 1];            // QProfile (100 x 5 x 5) + the pad code's entries; the position-indexed Profile stays in global memory
    __shared__ double s_nprob[kQ ? kQNoiseProbLds : 8];
    __shared__ double s_prof[kUpdate ? (kQ ? 2500 : kProfLds) : 1];
    __shared__ double s_noise[kUpdate ? kNoiseLds : 1];
    __shared__ double s_rspd[kUpdate ? kRspdLds : 1];
    __shared__ double s_gld[kUpdate ? kGldLds : 1];
    __shared__ Shape s_shapes[kPlaneShapesMax];              // the EM layout's shape table (every read looks its shape up)
    if (PO.rank) {
        for (int i = threadIdx.x; i < PO.n_shapes && i < kPlaneShapesMax; i += blockDim.x) s_shapes[i] = PO.shapes[i];
        PO.shapes = s_shapes;
    }
    // (quality models: what the pad code of the positions past a read's end selects is 1 -- model_block.hpp, kPadCode8)
    if (kQ) for (int i = threadIdx.x; i < kQProbLds; i += blockDim.x) s_prob[i] = i < 2500 ? T.prof[i] : 1.0;
    for (int i = threadIdx.x; i < (kQ ? kQNoiseProbLds : 5); i += blockDim.x) s_nprob[i] = i < (kQ ? 500 : 5) ? T.noise[i] : 1.0;
    constexpr int kProfCap = kQ ? 2500 : kProfLds;           // entries of the count table held in LDS (the rest: global atomics)
    if (kUpdate) {
        for (int i = threadIdx.x; i < kProfCap; i += blockDim.x) s_prof[i] = 0.0;
        for (int i = threadIdx.x; i < kNoiseLds; i += blockDim.x) s_noise[i] = 0.0;
        for (int i = threadIdx.x; i < kRspdLds; i += blockDim.x) s_rspd[i] = 0.0;
        for (int i = threadIdx.x; i < kGldLds; i += blockDim.x) s_gld[i] = 0.0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // chunks of kGroupChunk rows dealt to the workgroups round-robin; inside a chunk the workgroup's waves take 4 rows each per step
    const uint64_t waves_per_block = blockDim.x / 64;
    if (kGroupChunk > 0)
        model_group_rows<kQ, kPE, kUpdate, kWide>(D, T, theta, cp, ncp, A, kQ ? s_prob : T.prof, s_nprob, s_prof, s_noise, s_rspd, s_gld, (uint64_t)(threadIdx.x >> 6) * 4,
                                           waves_per_block * 4, lane, PO, (uint64_t)kGroupChunk, (uint64_t)blockIdx.x, (uint64_t)gridDim.x);
    else  // (measurement builds, -DRSEM_GROUP_CHUNK=0: the grid-wide stride of rounds 4-5)
        model_group_rows<kQ, kPE, kUpdate, kWide>(D, T, theta, cp, ncp, A, kQ ? s_prob : T.prof, s_nprob, s_prof, s_noise, s_rspd, s_gld,
                                           ((uint64_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6)) * 4, (uint64_t)gridDim.x * waves_per_block * 4, lane, PO);
    if (!kUpdate) return;
    __syncthreads();
    const int nprof = min(kProfCap, T.prof_rows * 25);
    for (int i = threadIdx.x; i < nprof; i += blockDim.x)
        if (s_prof[i] != 0.0) unsafeAtomicAdd(&A.prof[i], s_prof[i]);
    const int nnoise = kQ ? 500 : 5;
    for (int i = threadIdx.x; i < nnoise; i += blockDim.x)
        if (s_noise[i] != 0.0) unsafeAtomicAdd(&A.noise[i], s_noise[i]);
    if (A.rspd)
        for (int i = threadIdx.x; i < min(kRspdLds, T.B + 2); i += blockDim.x)
            if (s_rspd[i] != 0.0) unsafeAtomicAdd(&A.rspd[i], s_rspd[i]);
    if (A.gld)
        for (int i = threadIdx.x; i < min(kGldLds, A.gld0_ub - A.gld0_lb + 1); i += blockDim.x)
            if (s_gld[i] != 0.0) unsafeAtomicAdd(&A.gld[i], s_gld[i]);
}

__global__ void k_hit_rows(uint64_t N1, const uint64_t* __restrict__ row_ptr, uint32_t* hit_row) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N1) return;
    for (uint64_t j = row_ptr[i]; j < row_ptr[i + 1]; j++) hit_row[j] = (uint32_t)i;
}

template <typename T>
hipError_t dmalloc(T** p, size_t n) { return hipMalloc((void**)p, (n ? n : 1) * sizeof(T)); }

template <typename T>
int upload(T** d, const T* h, size_t n, hipStream_t st) {
    RSEM_HIP_TRY(dmalloc(d, n));
    if (n) return rsem::staged_h2d(*d, h, sizeof(T) * n, st);
    return RSEM_OK;
}

// reads arrive as one byte per base, back to back (offsets `off`, relative to off[0]); the kernels want every read on a
// 64-bit word boundary, 8 codes per word.  Lengths, word offsets (scan) and the repacking are done here on the device.
__global__ void k_read_words(uint64_t N1, const uint64_t* __restrict__ off, uint64_t* nwords, int32_t* len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > N1) return;
    if (i == N1) { nwords[i] = 0; return; }
    const uint64_t l = off[i + 1] - off[i];
    len[i] = (int32_t)l;
    nwords[i] = (l + 7) / 8;
}

__global__ void k_pack_reads(uint64_t N1, const uint64_t* __restrict__ off, const uint64_t* __restrict__ off8,
                             const uint8_t* __restrict__ raw, uint64_t* words) {
    // one wave per 64 reads would waste lanes on the short copy loops: thread per output word instead
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N1) return;
    const uint64_t b0 = off[i] - off[0], l = off[i + 1] - off[i];
    uint64_t* o = words + off8[i];
    for (uint64_t w = 0; w * 8 < l; w++) {
        uint64_t v = 0;
        const uint64_t n = l - w * 8 < 8 ? l - w * 8 : 8;
        for (uint64_t k = 0; k < n; k++) v |= (uint64_t)raw[b0 + w * 8 + k] << (8 * k);  // little-endian: byte k of the word
        o[w] = v;
    }
}

// Quality models: a read position becomes ONE 16-bit code (model_block.hpp, DevData).  `seq` / `qual` hold the mate's bases / qualities of
// all reads back to back; word w of `lo` takes positions 8w .. 8w + 3 of a read, word w of `hi` positions 8w + 4 .. 8w + 7, the pad code
// past the read's end.  A group of 16 lanes per read, a lane per word pair: the 8 + 8 input bytes of a word pair are two (unaligned) 8-byte
// loads, the stores of a group are contiguous.  (A thread per read with byte loads took 15 ms per launch at a fifth of configs[2].)
__global__ void k_code_reads(uint64_t N1, const uint64_t* __restrict__ off, const uint64_t* __restrict__ off8, const uint8_t* __restrict__ seq,
                             const uint8_t* __restrict__ qual, uint64_t* lo, uint64_t* hi) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i = t >> 4;
    if (i >= N1) return;
    const uint64_t b0 = off[i] - off[0], l = off[i + 1] - off[i], o8 = off8[i];
    for (uint64_t w = t & 15u; w * 8 < l; w += 16) {
        const uint64_t at = b0 + w * 8, n = l - w * 8 < 8 ? l - w * 8 : 8;
        uint64_t sb = 0, qb = 0;
        if (n == 8) {
            __builtin_memcpy(&sb, seq + at, 8);
            __builtin_memcpy(&qb, qual + at, 8);
        } else {
            for (uint64_t k = 0; k < n; k++) { sb |= (uint64_t)seq[at + k] << (8 * k); qb |= (uint64_t)qual[at + k] << (8 * k); }
        }
        uint64_t v[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint64_t c = (uint64_t)k < n ? (uint64_t)read_code8((unsigned)((qb >> (8 * k)) & 0xff), (unsigned)((sb >> (8 * k)) & 0xff)) : (uint64_t)kPadCode8;
            v[k >> 2] |= c << (16 * (k & 3));
        }
        lo[o8 + w] = v[0];
        hi[o8 + w] = v[1];
    }
}

}  // namespace

struct rsem_model_ctx {
    rsem_em_ctx* em = nullptr;
    bool holds_view = false;  // em_view_hold .. em_view_release
    rsem::EmDeviceView v;
    DevData D;
    DevTables T;
    bool have_tables = false;
    int B_alloc = 0, gld_n = 0, mld_n = 0, prof_n = 0, noise_n = 0;
    std::vector<void*> owned;       // device allocations of the immutable data
    uint32_t *d_aw0 = nullptr, *d_aw1 = nullptr, *d_afull = nullptr, *d_atot = nullptr;  // DevData::aw0 .. atot (owned)
    uint8_t *d_aw0h = nullptr, *d_aw1h = nullptr;  // DevData::aw0h / aw1h (owned; the wide path only)
    int addr_bits = 32;             // window_addr_bits of this context: 32 = the narrow instantiations, else the wide ones
    uint64_t strand_bytes = 0, strand_pad = 0;  // both strands of every transcript; RSEM_MODEL_STRAND_PAD
    uint8_t* d_flags = nullptr;     // DevData::same_prev, writable (bit 2 is set with the first tables: it needs the seed length)
    int fields_seedLen = -1;        // the seed length aw0 .. atot / bit 2 were computed with (-1: not yet)
    double* d_theta = nullptr;                // the round's theta for the weights of k_model_group, [M+1]
    int n_cus = 0;
    // table buffers (re-uploaded every round)
    double *t_rspd_pdf = nullptr, *t_rspd_cdf = nullptr, *t_gld_pdf = nullptr, *t_gld_cdf = nullptr, *t_mld_pdf = nullptr,
           *t_mld_cdf = nullptr, *t_prof = nullptr, *t_noise = nullptr, *t_mw = nullptr;
    // accumulators
    double *a_prof = nullptr, *a_noise = nullptr, *a_rspd = nullptr, *a_gld = nullptr;
    size_t a_prof_n = 0, a_gld_n = 0;
};

namespace {

template <typename T>
int up_field(rsem_model_ctx* c, const T*& field, const T* src, size_t n, hipStream_t st) {
    T* p = nullptr;
    int rc = upload(&p, src, n, st);
    if (rc != RSEM_OK) return rc;
    c->owned.push_back(p);
    field = p;
    return RSEM_OK;
}

// the group-per-read kernel: conprb + noise (+ weights and statistics when theta / accumulators are given).  (The thread-per-
// alignment and thread-per-read kernel families of rounds 2-3, kept behind RSEM_MODEL_KERNELS as cross-checks until round 5, left the
// product in round 6: the kernel body is checked on the CPU emulator and the programs against the reference's files.)
template <bool kQ, bool kPE, bool kWide>
int launch_group(rsem_model_ctx* c, const double* d_theta, const AccumPtrs* A, const PlaneOut& PO) {
    if (!c->D.N1) return RSEM_OK;
    if (!c->n_cus) {
        hipDeviceProp_t p;
        RSEM_HIP_TRY(hipGetDeviceProperties(&p, c->v.device));
        c->n_cus = std::max(1, p.multiProcessorCount);
    }
    const uint64_t chunks = kGroupChunk > 0 ? (c->D.N1 + kGroupChunk - 1) / kGroupChunk : (c->D.N1 + 31) / 32;
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)c->n_cus * 2, chunks));
    if (A)
        hipLaunchKernelGGL((k_model_group<kQ, kPE, true, kWide>), dim3(grid), dim3(kGroupBlk), 0, c->v.stream, c->D, c->T, d_theta, c->v.d_cp, c->v.d_ncp, *A, PO);
    else
        hipLaunchKernelGGL((k_model_group<kQ, kPE, false, kWide>), dim3(grid), dim3(kGroupBlk), 0, c->v.stream, c->D, c->T, (const double*)nullptr, c->v.d_cp,
                           c->v.d_ncp, AccumPtrs{nullptr, nullptr, nullptr, nullptr, 0, 0}, PO);
    RSEM_HIP_TRY(hipGetLastError());
    return RSEM_OK;
}
// The round kernel, then the EM context's planes: written in place by the kernel where the layout takes doubles (the
// default), else (Q32 planes, RSEM_MODEL_PLANES=0) refreshed from the CSR by the scatter pass.
int launch_group_any(rsem_model_ctx* c, const double* d_theta, const AccumPtrs* A) {
    PlaneOut PO{nullptr, nullptr, 0, 0, 0, nullptr, nullptr};
    rsem::EmPlanesView pv;
    const char* e = getenv("RSEM_MODEL_PLANES");
    bool in_place = !(e && !strcmp(e, "0")) && rsem::em_planes_writable(c->em);  // (a question: a layout of Q32 planes or split rows is no error)
    if (in_place) {
        const int vrc = rsem::em_planes_view(c->em, &pv);
        if (vrc != RSEM_OK) return vrc;
    }
    if (in_place && pv.n_shapes > kPlaneShapesMax) {  // (cannot happen: kMaxShapes == kShapeTableMax; the kernel's LDS copy holds no more)
        rsem::set_last_error("the EM layout has %d shapes, the model kernel's table holds %d", pv.n_shapes, kPlaneShapesMax);
        return RSEM_ERR_STATE;
    }
    if (in_place) PO = PlaneOut{pv.d_rank, (const Shape*)pv.d_shapes, pv.n_shapes, pv.T, pv.n_sell_rows, pv.d_sval, pv.d_sncp};
    int rc;
    // (the instantiation was chosen once, at create: window_addr_bits)
    if (c->addr_bits == 32)
        switch (c->D.model_type) {
            case 0: rc = launch_group<false, false, false>(c, d_theta, A, PO); break;
            case 1: rc = launch_group<true, false, false>(c, d_theta, A, PO); break;
            case 2: rc = launch_group<false, true, false>(c, d_theta, A, PO); break;
            default: rc = launch_group<true, true, false>(c, d_theta, A, PO); break;
        }
    else
        switch (c->D.model_type) {
            case 0: rc = launch_group<false, false, true>(c, d_theta, A, PO); break;
            case 1: rc = launch_group<true, false, true>(c, d_theta, A, PO); break;
            case 2: rc = launch_group<false, true, true>(c, d_theta, A, PO); break;
            default: rc = launch_group<true, true, true>(c, d_theta, A, PO); break;
        }
    if (rc != RSEM_OK) return rc;
    return in_place ? rsem::em_values_written_in_place(c->em) : rsem::em_values_changed(c->em);
}

int resize_buf(double** p, int* cur, int n) {
    if (*p && *cur >= n) return RSEM_OK;
    if (*p) hipFree(*p);
    *p = nullptr;
    RSEM_HIP_TRY(dmalloc(p, (size_t)n));
    *cur = n;
    return RSEM_OK;
}

}  // namespace

extern "C" {

int rsem_model_destroy(rsem_model_ctx* c) {
    if (!c) return RSEM_OK;
    (void)hipSetDevice(c->v.device);
    if (c->em && c->holds_view) rsem::em_view_release(c->em);
    for (void* p : c->owned) hipFree(p);
    hipFree(c->d_aw0); hipFree(c->d_aw1); hipFree(c->d_afull); hipFree(c->d_atot); hipFree(c->d_aw0h); hipFree(c->d_aw1h);
    hipFree(c->t_rspd_pdf); hipFree(c->t_rspd_cdf); hipFree(c->t_gld_pdf); hipFree(c->t_gld_cdf); hipFree(c->t_mld_pdf);
    hipFree(c->t_mld_cdf); hipFree(c->t_prof); hipFree(c->t_noise); hipFree(c->t_mw);
    hipFree(c->a_prof); hipFree(c->a_noise); hipFree(c->a_rspd); hipFree(c->a_gld);
    hipFree(c->d_theta);
    delete c;
    return RSEM_OK;
}

int rsem_model_create(rsem_model_ctx** out, rsem_em_ctx* em, const rsem_model_data* d) {
    RSEM_REQUIRE(out && em && d, "NULL argument");
    *out = nullptr;
    RSEM_REQUIRE(d->model_type >= 0 && d->model_type <= 3, "model_type must be 0..3");
    const bool q = d->model_type == 1 || d->model_type == 3, pe = d->model_type >= 2;
    RSEM_REQUIRE(d->row_ptr && d->sid_signed && d->pos && d->read_off[0] && d->read_seq[0] && d->low_quality && d->ref_off &&
                     d->ref_seq && d->fullLen && d->totLen && d->mask_off && d->mask_words,
                 "NULL array in rsem_model_data");
    RSEM_REQUIRE(!pe || (d->insertL && d->read_off[1] && d->read_seq[1]), "paired-end data needs insertL and mate 2");
    RSEM_REQUIRE(!q || (d->read_qual[0] && (!pe || d->read_qual[1])), "quality models need read_qual");
    // How the strand array will be addressed (window_addr_bits), decided before anything is built or uploaded.
    // RSEM_MODEL_STRAND_PAD (a test seam): that many bytes in front of the strands on the device -- allocated,
    // never written, never read -- so that kilobytes of input have window addresses above 2^32.
    uint64_t strand_pad = 0, strand_bytes = 0;
    if (const char* e = getenv("RSEM_MODEL_STRAND_PAD")) {
        char* end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        RSEM_REQUIRE(end != e && *end == '\0' && e[0] >= '0' && e[0] <= '9' && v % 8 == 0, "RSEM_MODEL_STRAND_PAD must be a whole number of bytes, a multiple of 8");
        strand_pad = v;
    }
    for (int sid = 1; sid <= d->M; sid++) {
        RSEM_REQUIRE(d->totLen[sid] >= 0, "negative transcript length");
        strand_bytes += 2 * (((uint64_t)d->totLen[sid] + 7) / 8 * 8);
    }
    const int addr_bits = window_addr_bits(strand_bytes, strand_pad);
    if (!addr_bits) {
        rsem::set_last_error("the transcript sequences take %llu bytes on both strands (+ %llu bytes of RSEM_MODEL_STRAND_PAD): the model context addresses them with at most %d bits",
                             (unsigned long long)strand_bytes, (unsigned long long)strand_pad, kWideAddrBits);
        return RSEM_ERR_INVALID;
    }
    rsem_model_ctx* c = new (std::nothrow) rsem_model_ctx();
    if (!c) return RSEM_ERR_NOMEM;
    c->em = em;
    c->addr_bits = addr_bits;
    c->strand_bytes = strand_bytes;
    c->strand_pad = strand_pad;
    int rc = rsem::em_device_view(em, &c->v);
    if (rc != RSEM_OK) { delete c; return rc; }
    rsem::em_view_hold(em);
    c->holds_view = true;
    if (c->v.N1 != d->N1 || c->v.nnz != d->nnz || c->v.M != d->M) {
        rsem_model_destroy(c);  // (gives the view back: a held view refuses every later release_csr of the EM context)
        rsem::set_last_error("model data does not match the EM context (N1/nnz/M)");
        return RSEM_ERR_INVALID;
    }
    hipStream_t st = c->v.stream;
    DevData& D = c->D;
    memset(&D, 0, sizeof(D));
    D.model_type = d->model_type; D.M = d->M; D.N1 = d->N1; D.nnz = d->nnz;
    D.row_ptr = c->v.d_row_ptr;
#define UP(field, src, n)                                           \
    do {                                                            \
        rc = up_field(c, D.field, src, (size_t)(n), st);            \
        if (rc != RSEM_OK) { rsem_model_destroy(c); return rc; }    \
    } while (0)
    // both strands of every transcript as base ids (RefSeq::get_id, RefSeq.h:84-87), word-aligned starts, one spare word at the end:
    // host work that depends on the reference alone -- on threads of its own while the alignments and reads go up
    std::vector<uint64_t> soff(2 * ((size_t)d->M + 1), 0);
    uint64_t tot = 0;
    for (int sid = 1; sid <= d->M; sid++)
        for (int dir = 0; dir < 2; dir++) {
            soff[2 * sid + dir] = tot;
            tot += ((uint64_t)d->totLen[sid] + 7) / 8 * 8;
        }
    std::vector<uint8_t> strands;
    std::thread strand_builder([&]() {
        strands.assign(tot + 16, 0);
        const int nt = d->M > 2000 ? 16 : 1;
        std::vector<std::thread> th;
        for (int t = 0; t < nt; t++)
            th.emplace_back([&, t]() {
                for (int sid = 1 + t; sid <= d->M; sid += nt) {
                    const uint8_t* f = d->ref_seq + d->ref_off[sid];
                    const int tl = d->totLen[sid];
                    uint8_t* o0 = strands.data() + soff[2 * sid];
                    uint8_t* o1 = strands.data() + soff[2 * sid + 1];
                    memcpy(o0, f, (size_t)tl);
                    for (int p = 0; p < tl; p++) {
                        const uint8_t b = f[tl - p - 1];
                        o1[p] = b == 4 ? 4 : 3 - b;  // get_rbase_id (utils.h:52-66)
                    }
                }
            });
        for (auto& x : th) x.join();
    });
    struct StrandJoin { std::thread& t; ~StrandJoin() { if (t.joinable()) t.join(); } } strand_join{strand_builder};  // (every early return)
    UP(sid_signed, d->sid_signed, d->nnz);
    UP(pos, d->pos, d->nnz);
    if (pe) UP(insertL, d->insertL, d->nnz);
    // reads: 8 codes per 64-bit word, every read on a word boundary (the kernels fetch 8 bases per load).  The bytes go
    // up as they are (pinned staging, upload.hpp) and are repacked on the device.
    for (int m = 0; m < (pe ? 2 : 1); m++) {
        const uint64_t b_lo = d->read_off[m][0], nbytes = d->read_off[m][d->N1] - b_lo;
        uint64_t *d_off = nullptr, *d_nw = nullptr, *d_off8 = nullptr, *d_ws = nullptr, *d_wq = nullptr;
        int32_t* d_len = nullptr;
        uint8_t *d_raw = nullptr, *d_raw_q = nullptr;
        void* d_tmp = nullptr;
        auto drop = [&]() { hipFree(d_off); hipFree(d_nw); hipFree(d_raw); hipFree(d_raw_q); hipFree(d_tmp); };
        auto bail = [&](int code) { drop(); hipFree(d_off8); hipFree(d_len); hipFree(d_ws); hipFree(d_wq); rsem_model_destroy(c); return code; };
        if ((rc = upload(&d_off, d->read_off[m], (size_t)d->N1 + 1, st)) != RSEM_OK) return bail(rc);
        if (dmalloc(&d_nw, (size_t)d->N1 + 1) != hipSuccess || dmalloc(&d_off8, (size_t)d->N1 + 1) != hipSuccess ||
            dmalloc(&d_len, (size_t)d->N1) != hipSuccess || dmalloc(&d_raw, (size_t)nbytes) != hipSuccess)
            return bail(RSEM_ERR_NOMEM);
        hipLaunchKernelGGL(k_read_words, dim3(rsem::ceil_div(d->N1 + 1, kBlk)), dim3(kBlk), 0, st, d->N1, d_off, d_nw, d_len);
        size_t tb = 0;
        if (hipcub::DeviceScan::ExclusiveSum(nullptr, tb, d_nw, d_off8, d->N1 + 1, st) != hipSuccess || hipMalloc(&d_tmp, tb ? tb : 1) != hipSuccess ||
            hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, d_nw, d_off8, d->N1 + 1, st) != hipSuccess)
            return bail(RSEM_ERR_HIP);
        uint64_t nw = 0;
        if (hipMemcpyAsync(&nw, d_off8 + d->N1, sizeof(uint64_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return bail(RSEM_ERR_HIP);
        nw += 1;  // one spare word: the last read's 8-byte fetches may look one word ahead
        for (int what = 0; what < (q ? 2 : 1); what++) {
            uint64_t*& d_w = what ? d_wq : d_ws;
            if (dmalloc(&d_w, (size_t)nw) != hipSuccess) return bail(RSEM_ERR_NOMEM);
            if (hipMemsetAsync(d_w + (nw - 1), 0, sizeof(uint64_t), st) != hipSuccess) return bail(RSEM_ERR_HIP);
        }
        // without qualities: the bases, 8 per word.  With: a position's base and quality become one 16-bit code (k_code_reads), from both
        // byte arrays at once (a second staging array for the qualities, freed with the first)
        if ((rc = rsem::staged_h2d(d_raw, d->read_seq[m] + b_lo, (size_t)nbytes, st)) != RSEM_OK) return bail(rc);
        if (q) {
            if (dmalloc(&d_raw_q, (size_t)nbytes) != hipSuccess) return bail(RSEM_ERR_NOMEM);
            if ((rc = rsem::staged_h2d(d_raw_q, d->read_qual[m] + b_lo, (size_t)nbytes, st)) != RSEM_OK) return bail(rc);
        }
        if (d->N1) {
            if (!q) hipLaunchKernelGGL(k_pack_reads, dim3(rsem::ceil_div(d->N1, kBlk)), dim3(kBlk), 0, st, d->N1, d_off, d_off8, d_raw, d_ws);
            else hipLaunchKernelGGL(k_code_reads, dim3(rsem::ceil_div(d->N1 * 16, kBlk)), dim3(kBlk), 0, st, d->N1, d_off, d_off8, d_raw, d_raw_q, d_ws, d_wq);
        }
        if (hipGetLastError() != hipSuccess) return bail(RSEM_ERR_HIP);
        if (hipStreamSynchronize(st) != hipSuccess) return bail(RSEM_ERR_HIP);
        drop();
        c->owned.push_back(d_off8); D.roff8[m] = d_off8;
        c->owned.push_back(d_len); D.rlen[m] = d_len;
        c->owned.push_back(d_ws); D.rseq_w[m] = d_ws;
        if (q) { c->owned.push_back(d_wq); D.rqual_w[m] = d_wq; }
    }
    UP(lq, d->low_quality, d->N1);
    {   // both strands of every transcript (built beside the uploads above: strand_builder)
        strand_builder.join();
        // (the device's offsets and every window address count from the start of the allocation: the pad lies in front)
        std::vector<uint64_t> soff_dev(soff);
        for (int sid = 1; sid <= d->M; sid++) { soff_dev[2 * sid] += strand_pad; soff_dev[2 * sid + 1] += strand_pad; }
        UP(soff, soff_dev.data(), soff_dev.size());
        uint8_t* wptr = nullptr;
        if (dmalloc(&wptr, (size_t)(strand_pad + tot + 16)) != hipSuccess) { rsem_model_destroy(c); return RSEM_ERR_NOMEM; }
        c->owned.push_back(wptr);
        rc = rsem::staged_h2d(wptr + strand_pad, strands.data(), (size_t)(tot + 16), st);
        if (rc != RSEM_OK) { rsem_model_destroy(c); return rc; }
        D.refw = reinterpret_cast<const uint64_t*>(wptr);
        if (hipStreamSynchronize(st) != hipSuccess) { rsem_model_destroy(c); return RSEM_ERR_HIP; }
    }
    UP(fullLen, d->fullLen, (size_t)d->M + 1);
    UP(totLen, d->totLen, (size_t)d->M + 1);
    UP(mask_off, d->mask_off, (size_t)d->M + 2);
    UP(mask_words, d->mask_words, d->mask_off[d->M + 1]);
#undef UP
    uint32_t* hr = nullptr;
    if (dmalloc(&hr, d->nnz) != hipSuccess) { rsem_model_destroy(c); return RSEM_ERR_NOMEM; }
    c->owned.push_back(hr);
    D.hit_row = hr;
    if (d->N1) hipLaunchKernelGGL(k_hit_rows, dim3(rsem::ceil_div(d->N1, kBlk)), dim3(kBlk), 0, st, d->N1, D.row_ptr, hr);
    uint8_t* fl = nullptr;
    if (dmalloc(&fl, d->nnz) != hipSuccess) { rsem_model_destroy(c); return RSEM_ERR_NOMEM; }
    c->owned.push_back(fl);
    D.same_prev = fl;
    c->d_flags = fl;
    {   // the strand array is addressed with 32 bits per alignment (DevData::aw0 / aw1), on the wide path with a byte more each
        const bool wide = c->addr_bits != 32;
        if (dmalloc(&c->d_aw0, d->nnz) != hipSuccess || (pe && dmalloc(&c->d_aw1, d->nnz) != hipSuccess) || dmalloc(&c->d_afull, d->nnz) != hipSuccess ||
            dmalloc(&c->d_atot, d->nnz) != hipSuccess || (wide && dmalloc(&c->d_aw0h, d->nnz) != hipSuccess) ||
            (wide && pe && dmalloc(&c->d_aw1h, d->nnz) != hipSuccess)) { rsem_model_destroy(c); return RSEM_ERR_NOMEM; }
        D.aw0 = c->d_aw0; D.aw1 = c->d_aw1; D.afull = c->d_afull; D.atot = c->d_atot; D.aw0h = c->d_aw0h; D.aw1h = c->d_aw1h;
    }
    if (d->nnz) {
        if (pe) hipLaunchKernelGGL(k_window_flags<true>, dim3(rsem::ceil_div(d->nnz, kBlk)), dim3(kBlk), 0, st, D, fl);
        else hipLaunchKernelGGL(k_window_flags<false>, dim3(rsem::ceil_div(d->nnz, kBlk)), dim3(kBlk), 0, st, D, fl);
    }
    if (hipStreamSynchronize(st) != hipSuccess) { rsem_model_destroy(c); return RSEM_ERR_HIP; }
    rsem::thread_stager().release();
    *out = c;
    return RSEM_OK;
}

int rsem_model_set_tables(rsem_model_ctx* c, const rsem_model_tables* t) {
    RSEM_REQUIRE(c && t && t->gld_pdf && t->gld_cdf && t->prof && t->noise && t->mw && t->rspd_pdf && t->rspd_cdf, "NULL table");
    RSEM_REQUIRE(!t->has_mld || (t->mld_pdf && t->mld_cdf), "mld tables missing");
    RSEM_REQUIRE(c->D.model_type < 2 || t->has_mld, "paired-end models need the mate length distribution");
    RSEM_HIP_TRY(hipSetDevice(c->v.device));
    hipStream_t st = c->v.stream;
    const bool q = c->D.model_type == 1 || c->D.model_type == 3;
    const int nr = t->B + 2, ng = t->gld_ub - t->gld_lb + 1, nm = t->has_mld ? t->mld_ub - t->mld_lb + 1 : 1;
    const int np = t->prof_rows * 25, nn = q ? 500 : 5;
    int rc;
    int cur;
    cur = c->B_alloc; if ((rc = resize_buf(&c->t_rspd_pdf, &cur, nr)) != RSEM_OK) return rc;
    if ((rc = resize_buf(&c->t_rspd_cdf, &c->B_alloc, nr)) != RSEM_OK) return rc;
    cur = c->gld_n; if ((rc = resize_buf(&c->t_gld_pdf, &cur, ng)) != RSEM_OK) return rc;
    if ((rc = resize_buf(&c->t_gld_cdf, &c->gld_n, ng)) != RSEM_OK) return rc;
    cur = c->mld_n; if ((rc = resize_buf(&c->t_mld_pdf, &cur, nm)) != RSEM_OK) return rc;
    if ((rc = resize_buf(&c->t_mld_cdf, &c->mld_n, nm)) != RSEM_OK) return rc;
    if ((rc = resize_buf(&c->t_prof, &c->prof_n, np)) != RSEM_OK) return rc;
    if ((rc = resize_buf(&c->t_noise, &c->noise_n, nn)) != RSEM_OK) return rc;
    if (!c->t_mw) RSEM_HIP_TRY(dmalloc(&c->t_mw, (size_t)c->D.M + 1));
    auto cp = [&](double* dst, const double* src, int n) { return hipMemcpyAsync(dst, src, sizeof(double) * n, hipMemcpyHostToDevice, st); };
    RSEM_HIP_TRY(cp(c->t_rspd_pdf, t->rspd_pdf, nr));
    RSEM_HIP_TRY(cp(c->t_rspd_cdf, t->rspd_cdf, nr));
    RSEM_HIP_TRY(cp(c->t_gld_pdf, t->gld_pdf, ng));
    RSEM_HIP_TRY(cp(c->t_gld_cdf, t->gld_cdf, ng));
    if (t->has_mld) {
        RSEM_HIP_TRY(cp(c->t_mld_pdf, t->mld_pdf, nm));
        RSEM_HIP_TRY(cp(c->t_mld_cdf, t->mld_cdf, nm));
    }
    RSEM_HIP_TRY(cp(c->t_prof, t->prof, np));
    RSEM_HIP_TRY(cp(c->t_noise, t->noise, nn));
    RSEM_HIP_TRY(cp(c->t_mw, t->mw, c->D.M + 1));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    DevTables& T = c->T;
    T.probF = t->probF; T.seedLen = t->seedLen; T.estRSPD = t->estRSPD; T.B = t->B;
    T.rspd_pdf = c->t_rspd_pdf; T.rspd_cdf = c->t_rspd_cdf;
    T.gld_lb = t->gld_lb; T.gld_ub = t->gld_ub; T.gld_pdf = c->t_gld_pdf; T.gld_cdf = c->t_gld_cdf;
    T.has_mld = t->has_mld; T.mld_lb = t->mld_lb; T.mld_ub = t->mld_ub; T.mld_pdf = c->t_mld_pdf; T.mld_cdf = c->t_mld_cdf;
    T.prof_rows = t->prof_rows; T.prof = c->t_prof; T.noise = c->t_noise; T.mw = c->t_mw;
    if (c->fields_seedLen != t->seedLen) {  // (once per context in the programs: the seed length is a constant of the model)
        if (c->D.nnz) {
            const bool pe = c->D.model_type >= 2, wide = c->addr_bits != 32;
            const dim3 grid(rsem::ceil_div(c->D.nnz, kBlk));
#define FIELDS(PE, WIDE)                                                                                                                                  \
    hipLaunchKernelGGL((k_alignment_fields<PE, WIDE>), grid, dim3(kBlk), 0, st, c->D, t->seedLen, c->d_aw0, c->d_aw1, c->d_afull, c->d_atot, c->d_flags, \
                       c->d_aw0h, c->d_aw1h)
            if (!wide) { if (pe) FIELDS(true, false); else FIELDS(false, false); }
            else { if (pe) FIELDS(true, true); else FIELDS(false, true); }
#undef FIELDS
            RSEM_HIP_TRY(hipGetLastError());
            RSEM_HIP_TRY(hipStreamSynchronize(st));
        }
        c->fields_seedLen = t->seedLen;
    }
    c->have_tables = true;
    return RSEM_OK;
}

int rsem_model_calc_conprb(rsem_model_ctx* c) {
    RSEM_REQUIRE(c, "NULL argument");
    if (!c->have_tables) { rsem::set_last_error("model tables were never set"); return RSEM_ERR_STATE; }
    RSEM_HIP_TRY(hipSetDevice(c->v.device));
    return launch_group_any(c, nullptr, nullptr);
}

int rsem_model_estep_update(rsem_model_ctx* c, const double* theta, double N0, double* counts, double* theta_new, double* sum,
                            double* bChange, int32_t* totNum, rsem_model_accum* acc) {
    // (Kept for callers of the two-call form -- rsem_model_calc_conprb, then this.  Since round 6 it IS the one-pass round: the
    // kernel recomputes the probabilities from the tables last set -- the same values rsem_model_calc_conprb left -- on its way to
    // the weights and the statistics.)
    RSEM_REQUIRE(c && theta && acc && acc->prof && acc->noise, "NULL argument");
    return rsem_model_round(c, theta, N0, counts, theta_new, sum, bChange, totNum, acc);
}

// One model round in one pass over the reads (rounds 1-11 of EM.cpp:383-404): alignment probabilities with the tables last
// set, the E step's posterior weights for `theta` and -- when `acc` is given (rounds 1-10) -- the model's statistics, all
// by k_model_group; then the round's counts / theta / convergence numbers from the E-step kernel on the refreshed planes.
int rsem_model_round(rsem_model_ctx* c, const double* theta, double N0, double* counts, double* theta_new, double* sum,
                     double* bChange, int32_t* totNum, rsem_model_accum* acc) {
    RSEM_REQUIRE(c && theta, "NULL argument");
    if (!c->have_tables) { rsem::set_last_error("model tables were never set"); return RSEM_ERR_STATE; }
    const bool q = c->D.model_type == 1 || c->D.model_type == 3, pe = c->D.model_type >= 2;
    RSEM_REQUIRE(!acc || (acc->prof && acc->noise), "NULL accumulator");
    RSEM_REQUIRE(!acc || !pe || acc->gld, "paired-end models accumulate the fragment length distribution");
    RSEM_REQUIRE(!acc || !c->T.estRSPD || acc->rspd, "estRSPD needs the rspd accumulator");
    RSEM_HIP_TRY(hipSetDevice(c->v.device));
    hipStream_t st = c->v.stream;
    int rc;
    const size_t np = (size_t)c->T.prof_rows * 25, nn = q ? 500 : 5, nr = (size_t)c->T.B + 2;
    const size_t ng = (acc && pe) ? (size_t)(acc->gld0_ub - acc->gld0_lb + 1) : 1;
    if (acc) {
        if (!c->d_theta) RSEM_HIP_TRY(dmalloc(&c->d_theta, (size_t)c->D.M + 1));
        RSEM_HIP_TRY(hipMemcpyAsync(c->d_theta, theta, sizeof(double) * ((size_t)c->D.M + 1), hipMemcpyHostToDevice, st));
        if (c->a_prof_n < np) { hipFree(c->a_prof); c->a_prof = nullptr; RSEM_HIP_TRY(dmalloc(&c->a_prof, np)); c->a_prof_n = np; }
        if (!c->a_noise) RSEM_HIP_TRY(dmalloc(&c->a_noise, (size_t)500));
        if (!c->a_rspd) RSEM_HIP_TRY(dmalloc(&c->a_rspd, std::max<size_t>(nr, 1024)));
        if (c->a_gld_n < ng) { hipFree(c->a_gld); c->a_gld = nullptr; RSEM_HIP_TRY(dmalloc(&c->a_gld, ng)); c->a_gld_n = ng; }
        RSEM_HIP_TRY(hipMemsetAsync(c->a_prof, 0, sizeof(double) * np, st));
        RSEM_HIP_TRY(hipMemsetAsync(c->a_noise, 0, sizeof(double) * 500, st));
        RSEM_HIP_TRY(hipMemsetAsync(c->a_rspd, 0, sizeof(double) * nr, st));
        RSEM_HIP_TRY(hipMemsetAsync(c->a_gld, 0, sizeof(double) * ng, st));
        AccumPtrs A{c->a_prof, c->a_noise, c->T.estRSPD ? c->a_rspd : nullptr, pe ? c->a_gld : nullptr, acc->gld0_lb, acc->gld0_ub};
        rc = launch_group_any(c, c->d_theta, &A);
    } else {
        rc = launch_group_any(c, nullptr, nullptr);
    }
    if (rc != RSEM_OK) return rc;
    rc = rsem_em_step(c->em, theta, N0, counts, theta_new, sum, bChange, totNum);
    if (rc != RSEM_OK) return rc;
    if (acc) {
        RSEM_HIP_TRY(hipMemcpyAsync(acc->prof, c->a_prof, sizeof(double) * np, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(acc->noise, c->a_noise, sizeof(double) * nn, hipMemcpyDeviceToHost, st));
        if (c->T.estRSPD) RSEM_HIP_TRY(hipMemcpyAsync(acc->rspd, c->a_rspd, sizeof(double) * nr, hipMemcpyDeviceToHost, st));
        if (pe) RSEM_HIP_TRY(hipMemcpyAsync(acc->gld, c->a_gld, sizeof(double) * ng, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
    }
    return RSEM_OK;
}

int rsem_model_get_info(const rsem_model_ctx* c, const char* key, int64_t* value) {
    RSEM_REQUIRE(c && key && value, "NULL argument");
    if (!strcmp(key, "window_addr_bits")) *value = c->addr_bits;
    else if (!strcmp(key, "strand_bytes")) *value = (int64_t)c->strand_bytes;
    else if (!strcmp(key, "strand_pad_bytes")) *value = (int64_t)c->strand_pad;
    else { rsem::set_last_error("unknown info key '%s'", key); return RSEM_ERR_INVALID; }
    return RSEM_OK;
}

int rsem_model_get_values(rsem_model_ctx* c, double* conprb, double* ncp) {
    RSEM_REQUIRE(c && conprb && ncp, "NULL argument");
    RSEM_HIP_TRY(hipSetDevice(c->v.device));
    if (c->v.nnz) RSEM_HIP_TRY(hipMemcpyAsync(conprb, c->v.d_cp, sizeof(double) * c->v.nnz, hipMemcpyDeviceToHost, c->v.stream));
    if (c->v.N1) RSEM_HIP_TRY(hipMemcpyAsync(ncp, c->v.d_ncp, sizeof(double) * c->v.N1, hipMemcpyDeviceToHost, c->v.stream));
    RSEM_HIP_TRY(hipStreamSynchronize(c->v.stream));
    return RSEM_OK;
}

}  // extern "C"

// rsem_hip_preload (status.hip): the first launch of a translation unit makes the runtime load its code object
namespace { __global__ void k_preload_model() {} }
namespace rsem { void preload_model() { hipLaunchKernelGGL(k_preload_model, dim3(1), dim3(1), 0, nullptr); (void)hipGetLastError(); } }
