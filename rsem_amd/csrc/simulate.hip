// simulate.hip -- the loop of rsem-simulate-reads on MI355X.  Replaces simulation.cpp:121-126: per read,
// model.simulate until it gives a read, the counts and the resimulation total.  One attempt is attempt<> of simulate_block.hpp.
//
// rsem_sim_counter_batch: one kernel.
//   k_sim_counter       a lane per read: its own attempts, each on its own Philox counter, until one gives a read or the cap is met.
// rsem_sim_reference_batch: the one MT19937 stream, produced on the host (the twist is sequential: 2.4 ns a word on one thread) and
// searched in chunks of n_pos positions with the longest attempt's words behind them; a chunk's entry is always its word 0:
//   k_sim_heads         a lane per position p: the attempt that WOULD begin at p, its uniforms counted, nothing written but
//                       next_ok[p] = p + uniforms | gives-a-read << 31;
//   k_sim_tile_exits    a workgroup per tile: next_ok of the tile into LDS, one backward sweep (tile_exits): every position's exit;
//   k_sim_hop           one lane: from word 0 tile to tile through the exits; the entry of every tile the stream passes, the chunk's exit;
//   k_sim_mark          a workgroup per tile, its lane 0: from the tile's entry along next_ok, a flag word per visited position
//                       (a read: 1, a failed attempt: 1 << 32);
//   hipcub::DeviceScan::ExclusiveSum   reads and failed attempts before every position;
//   k_sim_starts        a lane per position: a visited read's position into starts[its ordinal];
//   k_sim_body          a lane per read: the attempt at starts[j] again, now writing; the failed attempts since the read before.
// Words with more than one writer: the per-transcript counts (vector atomics on 64-bit integers) and the status word (atomicMax).
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cmath>
#include <mutex>
#include <vector>

#include "host/ci_stream.hpp"
#include "simt_macros.hpp"
#include "simulate_block.hpp"
#include "stage_util.hpp"

using namespace rsem_simk;

namespace {

using rsem::blocks256;
using Buf = rsem::GrowBuf<4>;

constexpr uint32_t kNoEntry = 0xffffffffu;
constexpr uint32_t kMaxTile = 8192;
constexpr int kTileThreads = 64;

// what the kernels of a chunk hand to the host
struct ChunkState {
    uint32_t exit_pos;       // k_sim_hop: the first visited position at or behind n_pos
    uint32_t last_next;      // k_sim_body: the position behind the last read taken
    uint64_t last_fails;     // ... and the failed attempts before that read
    int32_t status;
    uint32_t pad;
};

// the output arrays of a batch on the device
struct Out {
    int32_t *sid, *dir, *pos, *insert_l, *len1, *len2;
    uint32_t* attempts;
    uint8_t *seq1, *qual1, *seq2, *qual2;
    int32_t stride;
};

enum { B_WORDS, B_NEXT, B_EXIT, B_FLAGS, B_SUMS, B_ENTRY, B_STARTS, B_TMP, B_I32, B_BYTES, B_COUNT };

// the quality models' small tables in LDS: qc_trans 80 000 bytes, pc 20 000, npc 4 000, qc_init 800
constexpr size_t kLdsDoubles = (size_t)kQ * kQ + (size_t)kQ * 25 + (size_t)kQ * 5 + kQ;

// every lane of the workgroup; the tables a quality model samples from move to `lds`
__device__ inline Tables stage_tables(const Tables& T, double* lds, bool use) {
    Tables L = T;
    if (!use) return L;
    double* trans = lds;
    double* pc = trans + kQ * kQ;
    double* npc = pc + kQ * 25;
    double* init = npc + kQ * 5;
    for (int i = RSEM_TIDX; i < kQ * kQ; i += RSEM_BDIM) trans[i] = T.qc_trans[i];
    for (int i = RSEM_TIDX; i < kQ * 25; i += RSEM_BDIM) pc[i] = T.pc[i];
    for (int i = RSEM_TIDX; i < kQ * 5; i += RSEM_BDIM) npc[i] = T.npc[i];
    for (int i = RSEM_TIDX; i < kQ; i += RSEM_BDIM) init[i] = T.qc_init[i];
    RSEM_SYNC();
    L.qc_trans = trans; L.pc = pc; L.npc = npc; L.qc_init = init;
    return L;
}

__device__ inline void write_read(const Out& o, int64_t j, const Attempt& a, uint32_t attempts) {
    o.sid[j] = a.sid; o.dir[j] = a.dir; o.pos[j] = a.pos; o.insert_l[j] = a.insert_l; o.len1[j] = a.len1; o.len2[j] = a.len2;
    o.attempts[j] = attempts;
}

__global__ void __launch_bounds__(256) k_sim_counter(Tables T, int lds_tables, uint64_t seed, uint64_t first_read, int64_t n, uint32_t cap, Out o,
                                                      unsigned long long* __restrict__ counts, unsigned long long* __restrict__ resim, int32_t* status) {
    extern __shared__ double lds[];
    const Tables L = stage_tables(T, lds, lds_tables != 0);
    const int64_t j = (int64_t)blockIdx.x * 256 + RSEM_TIDX;
    if (j >= n) return;
    const size_t at = (size_t)j * (size_t)o.stride;
    Attempt a;
    uint32_t failed = 0;
    for (;;) {
        CounterSource s(seed, first_read + (uint64_t)j, failed);
        attempt<true>(L, s, a, o.seq1 + at, o.qual1 + at, o.seq2 + at, o.qual2 + at);
        if (a.ok || a.status != kOk) break;
        if (++failed >= cap) { a.status = kAttemptCap; break; }
    }
    if (a.status != kOk) { atomicMax(status, a.status); return; }
    write_read(o, j, a, failed);
    atomicAdd(&counts[a.sid], 1ull);
    if (failed) atomicAdd(resim, (unsigned long long)failed);
}

__global__ void __launch_bounds__(256) k_sim_heads(Tables T, int lds_tables, const uint32_t* __restrict__ words, uint32_t n_words, uint32_t n_pos,
                                                    uint32_t* __restrict__ next_ok) {
    extern __shared__ double lds[];
    const Tables L = stage_tables(T, lds, lds_tables != 0);
    const uint32_t p = blockIdx.x * 256u + (uint32_t)RSEM_TIDX;
    if (p >= n_pos) return;
    WordSource s(words, n_words, p);
    Attempt a;
    attempt<false>(L, s, a, nullptr, nullptr, nullptr, nullptr);
    // (a status at a position the stream never visits means nothing: k_sim_body reports those of the visited ones.  An attempt that
    // would run past the words takes part as a failed one: n_words leaves the longest attempt's room behind n_pos)
    next_ok[p] = (p + (a.draws ? a.draws : 1u)) | ((a.ok || (a.status != kOk && a.status != kPastWords)) ? kOkBit : 0u);
}

__global__ void __launch_bounds__(kTileThreads) k_sim_tile_exits(const uint32_t* __restrict__ next_ok, uint32_t n_pos, uint32_t tile, uint32_t* __restrict__ exit_of,
                                                                  unsigned long long* __restrict__ flags, uint32_t* __restrict__ entry) {
    __shared__ uint32_t t_next[kMaxTile];
    const uint32_t t0 = blockIdx.x * tile, t1 = min(t0 + tile, n_pos);
    for (uint32_t p = t0 + RSEM_TIDX; p < t1; p += kTileThreads) { t_next[p - t0] = next_ok[p]; flags[p] = 0ull; }
    if (RSEM_TIDX == 0) {
        entry[blockIdx.x] = kNoEntry;
        if (blockIdx.x == 0) flags[n_pos] = 0ull;
    }
    RSEM_SYNC();
    if (RSEM_TIDX == 0) tile_exits_in_place(t_next, t0, t1);
    RSEM_SYNC();
    for (uint32_t p = t0 + RSEM_TIDX; p < t1; p += kTileThreads) exit_of[p] = t_next[p - t0];
}

__global__ void k_sim_hop(const uint32_t* __restrict__ exit_of, uint32_t n_pos, uint32_t tile, uint32_t* __restrict__ entry, ChunkState* st) {
    if (blockIdx.x || RSEM_TIDX) return;
    uint32_t p = 0;
    while (p < n_pos) {  // exit_of[p] > p: ends
        entry[p / tile] = p;
        p = exit_of[p];
    }
    st->exit_pos = p;
}

__global__ void __launch_bounds__(kTileThreads) k_sim_mark(const uint32_t* __restrict__ next_ok, uint32_t n_pos, uint32_t tile, const uint32_t* __restrict__ entry,
                                                            unsigned long long* __restrict__ flags) {
    if (RSEM_TIDX) return;
    uint32_t p = entry[blockIdx.x];
    if (p == kNoEntry) return;
    const uint32_t t1 = min(blockIdx.x * tile + tile, n_pos);
    while (p < t1) {
        const uint32_t w = next_ok[p];
        flags[p] = (w & kOkBit) ? 1ull : 1ull << 32;
        p = w & ~kOkBit;
    }
}

__global__ void __launch_bounds__(256) k_sim_starts(const unsigned long long* __restrict__ flags, const unsigned long long* __restrict__ sums, uint32_t n_pos,
                                                     uint32_t max_reads, uint32_t* __restrict__ starts) {
    const uint32_t p = blockIdx.x * 256u + (uint32_t)RSEM_TIDX;
    if (p >= n_pos || !(flags[p] & 0xffffffffull)) return;
    const uint32_t j = (uint32_t)(sums[p] & 0xffffffffull);
    if (j < max_reads) starts[j] = p;
}

__global__ void __launch_bounds__(256) k_sim_body(Tables T, int lds_tables, const uint32_t* __restrict__ words, uint32_t n_words, const uint32_t* __restrict__ starts,
                                                   const unsigned long long* __restrict__ sums, uint32_t n, uint32_t carry_fails, uint32_t cap, Out o, int64_t out_at,
                                                   unsigned long long* __restrict__ counts, ChunkState* st) {
    extern __shared__ double lds[];
    const Tables L = stage_tables(T, lds, lds_tables != 0);
    const uint32_t j = blockIdx.x * 256u + (uint32_t)RSEM_TIDX;
    if (j >= n) return;
    const uint32_t p = starts[j];
    const uint64_t fails_before = sums[p] >> 32;
    const uint64_t run = j ? fails_before - (sums[starts[j - 1]] >> 32) : fails_before + carry_fails;
    const int64_t r = out_at + j;
    const size_t at = (size_t)r * (size_t)o.stride;
    WordSource s(words, n_words, p);
    Attempt a;
    attempt<true>(L, s, a, o.seq1 + at, o.qual1 + at, o.seq2 + at, o.qual2 + at);
    if (a.status == kOk && !a.ok) a.status = kPastWords;  // the search saw a read here
    if (a.status == kOk && run >= cap) a.status = kAttemptCap;
    if (a.status != kOk) { atomicMax(&st->status, a.status); return; }
    write_read(o, r, a, (uint32_t)run);
    atomicAdd(&counts[a.sid], 1ull);
    if (j == n - 1) { st->last_next = p + a.draws; st->last_fails = fails_before; }
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

struct rsem_sim {
    int device = 0;
    Tables T{};             // pointers into device memory
    rsem::DevMem mem;       // the tables
    rsem::StageQueue q;
    hipEvent_t ed = nullptr;  // between search and body
    Buf buf[B_COUNT];
    size_t device_bytes = 0;
    unsigned long long* d_counts = nullptr;  // [M + 1], then the counter stream's failed attempts
    ChunkState* d_state = nullptr;
    uint64_t resimulations = 0;
    bool dead = false, begun = false;
    bool q_model = false;
    rsemh::RefMt19937 gen{0};  // boost::random::mt19937 as simul.h:11 seeds it
    std::vector<uint32_t> pending;  // generator words not yet consumed; the stream's next word is pending[0]
    uint64_t carry_fails = 0;       // failed attempts since the last read: in no total yet
    std::mutex mu;
};

namespace {

int read_knobs(rsem_sim_knobs* k) {
    k->batch_reads = 1ull << 18; k->chunk_words = 1ull << 22; k->tile = 2048; k->attempt_cap = kDefaultAttemptCap; k->lds_tables = 1;
    if (int rc = rsem::env_whole("RSEM_SIM_BATCH_READS", 1, 1ll << 30, &k->batch_reads)) return rc;
    if (int rc = rsem::env_whole("RSEM_SIM_CHUNK_WORDS", 1, 1ll << 30, &k->chunk_words)) return rc;
    if (int rc = rsem::env_whole("RSEM_SIM_TILE", 1, kMaxTile, &k->tile)) return rc;
    if (int rc = rsem::env_whole("RSEM_SIM_ATTEMPT_CAP", 1, 1ll << 31, &k->attempt_cap)) return rc;
    return rsem::env_whole("RSEM_SIM_LDS_TABLES", 0, 1, &k->lds_tables);
}

bool ascending(const double* a, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(a[i]) || a[i] < 0.0 || (i && a[i] < a[i - 1])) return false;
    return true;
}
bool rows_ascending(const double* a, size_t rows, size_t n) {
    for (size_t r = 0; r < rows; r++)
        if (!ascending(a + r * n, n)) return false;
    return true;
}

template <class T>
int upload(rsem_sim* h, const T** dst, const T* src, size_t n) {
    T* d = nullptr;
    RSEM_HIP_TRY(h->mem.alloc(&d, n));
    RSEM_HIP_TRY(hipMemcpy(d, src, n * sizeof(T), hipMemcpyHostToDevice));
    *dst = d;
    return RSEM_OK;
}

int check_batch(const rsem_sim* h, const rsem_sim_batch* b, int64_t n, const char* who) {
    if (!b) { rsem::set_last_error("%s: the batch must not be NULL", who); return RSEM_ERR_INVALID; }
    if (n < 0 || n >= (1ll << 30)) { rsem::set_last_error("%s: 0 to 2^30 - 1 reads are expected", who); return RSEM_ERR_INVALID; }
    if (b->capacity < n) { rsem::set_last_error("%s: a batch of capacity %lld for %lld reads", who, (long long)b->capacity, (long long)n); return RSEM_ERR_INVALID; }
    if (b->stride < h->T.max_len) { rsem::set_last_error("%s: a stride of %d bytes, the longest read has %d", who, b->stride, h->T.max_len); return RSEM_ERR_INVALID; }
    const bool q = h->T.has_q(), pe = h->T.paired();
    if (n && (!b->sid || !b->dir || !b->pos || !b->insert_l || !b->len1 || !b->len2 || !b->attempts || !b->seq1 || (q && !b->qual1) || (pe && !b->seq2) || (pe && q && !b->qual2))) {
        rsem::set_last_error("%s: the batch's arrays must not be NULL", who);
        return RSEM_ERR_INVALID;
    }
    return RSEM_OK;
}

// the device arrays of n reads at a stride
int device_out(rsem_sim* h, int64_t n, int32_t stride, Out& o) {
    const size_t n1 = (size_t)std::max<int64_t>(n, 1);
    RSEM_HIP_TRY(h->buf[B_I32].need(n1 * 4 * 7, h->device_bytes));
    RSEM_HIP_TRY(h->buf[B_BYTES].need(n1 * (size_t)stride * 4, h->device_bytes));
    int32_t* w = h->buf[B_I32].as<int32_t>();
    uint8_t* y = h->buf[B_BYTES].as<uint8_t>();
    o.sid = w; o.dir = w + n1; o.pos = w + 2 * n1; o.insert_l = w + 3 * n1; o.len1 = w + 4 * n1; o.len2 = w + 5 * n1; o.attempts = (uint32_t*)(w + 6 * n1);
    o.seq1 = y; o.qual1 = y + n1 * stride; o.seq2 = y + 2 * n1 * stride; o.qual2 = y + 3 * n1 * stride;
    o.stride = stride;
    return RSEM_OK;
}

int download(rsem_sim* h, const Out& o, int64_t n, rsem_sim_batch* b) {
    const double t0 = now_ms();
    hipStream_t st = h->q.st;
    const size_t w = (size_t)n * 4, y = (size_t)n * (size_t)o.stride;
    if (n) {
        RSEM_HIP_TRY(hipMemcpyAsync(b->sid, o.sid, w, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(b->dir, o.dir, w, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(b->pos, o.pos, w, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(b->insert_l, o.insert_l, w, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(b->len1, o.len1, w, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(b->len2, o.len2, w, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(b->attempts, o.attempts, w, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(b->seq1, o.seq1, y, hipMemcpyDeviceToHost, st));
        if (h->T.has_q()) RSEM_HIP_TRY(hipMemcpyAsync(b->qual1, o.qual1, y, hipMemcpyDeviceToHost, st));
        if (h->T.paired()) {
            RSEM_HIP_TRY(hipMemcpyAsync(b->seq2, o.seq2, y, hipMemcpyDeviceToHost, st));
            if (h->T.has_q()) RSEM_HIP_TRY(hipMemcpyAsync(b->qual2, o.qual2, y, hipMemcpyDeviceToHost, st));
        }
    }
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    b->download_ms += now_ms() - t0;
    return RSEM_OK;
}

size_t lds_bytes(const rsem_sim* h, const rsem_sim_knobs& k) { return (h->q_model && k.lds_tables) ? kLdsDoubles * sizeof(double) : 0; }

void clear_batch(rsem_sim_batch* b) {
    b->status = RSEM_SIM_OK; b->n_reads = 0; b->resimulations = 0; b->n_chunks = 0; b->n_launches = 0; b->stream_words = 0;
    b->words_ms = b->upload_ms = b->search_ms = b->body_ms = b->download_ms = 0.0;
}

}  // namespace

extern "C" int rsem_sim_read_knobs(rsem_sim_knobs* k) {
    RSEM_REQUIRE(k, "rsem_sim_read_knobs: k must not be NULL");
    return read_knobs(k);
}

extern "C" int rsem_sim_create(rsem_sim** out, const rsem_sim_model* m, int device) {
    RSEM_REQUIRE(out, "rsem_sim_create: out must not be NULL");
    *out = nullptr;
    RSEM_REQUIRE(m, "rsem_sim_create: the model must not be NULL");
    RSEM_REQUIRE(device >= 0, "rsem_sim_create: device must not be negative");
    RSEM_REQUIRE(m->type >= 0 && m->type <= 3, "rsem_sim_create: a model type from 0 to 3 is expected");
    RSEM_REQUIRE(m->M >= 1, "rsem_sim_create: M must be 1 or more");
    const bool q = m->type == 1 || m->type == 3, pe = m->type >= 2;
    RSEM_REQUIRE(m->theta_cdf && m->full_len && m->tot_len && m->seq_off && m->seq && m->g_cdf && m->pc && m->npc, "rsem_sim_create: a table is NULL");
    RSEM_REQUIRE(!pe || m->has_mld, "rsem_sim_create: a paired-end model has a mate-length distribution");
    RSEM_REQUIRE(!m->has_mld || m->m_cdf, "rsem_sim_create: m_cdf must not be NULL");
    RSEM_REQUIRE(!q || (m->qc_init && m->qc_trans), "rsem_sim_create: a quality model has qc_init and qc_trans");
    RSEM_REQUIRE(q || m->pro_len >= 1, "rsem_sim_create: pro_len must be 1 or more");
    RSEM_REQUIRE(!m->est_rspd || (m->B >= 1 && m->r_pdf && m->r_cdf), "rsem_sim_create: an estimated RSPD has B >= 1, r_pdf and r_cdf");
    RSEM_REQUIRE(m->g_lb >= 0 && m->g_lb < m->g_ub && m->g_ub < (1 << 24), "rsem_sim_create: 0 <= g_lb < g_ub < 2^24 is expected");
    RSEM_REQUIRE(!m->has_mld || (m->m_lb >= 0 && m->m_lb < m->m_ub && m->m_ub < (1 << 24)), "rsem_sim_create: 0 <= m_lb < m_ub < 2^24 is expected");
    RSEM_REQUIRE(m->prob_f >= 0.0 && m->prob_f <= 1.0, "rsem_sim_create: prob_f is a probability");
    RSEM_REQUIRE(m->seq_off[0] == 0 && m->seq_off[1] == 0, "rsem_sim_create: seq_off[0] and seq_off[1] must be 0");
    for (int i = 1; i <= m->M; i++)
        if (m->full_len[i] < 1 || m->full_len[i] > m->tot_len[i] || m->seq_off[i + 1] < m->seq_off[i] || m->seq_off[i + 1] - m->seq_off[i] < (uint64_t)m->tot_len[i]) {
            rsem::set_last_error("rsem_sim_create: transcript %d: 1 <= full_len <= tot_len and tot_len bytes of sequence are expected", i);
            return RSEM_ERR_INVALID;
        }
    RSEM_REQUIRE(ascending(m->theta_cdf, (size_t)m->M + 1), "rsem_sim_create: theta_cdf must be a finite running sum");
    RSEM_REQUIRE(m->g_cdf[0] == 0.0 && ascending(m->g_cdf, (size_t)(m->g_ub - m->g_lb) + 1), "rsem_sim_create: g_cdf must be a finite running sum from 0");
    RSEM_REQUIRE(m->g_cdf[m->g_ub - m->g_lb] > 0.0 && (!m->has_mld || m->m_cdf[m->m_ub - m->m_lb] > 0.0), "rsem_sim_create: a length distribution must have a total above 0");
    RSEM_REQUIRE(!m->has_mld || (m->m_cdf[0] == 0.0 && ascending(m->m_cdf, (size_t)(m->m_ub - m->m_lb) + 1)), "rsem_sim_create: m_cdf must be a finite running sum from 0");
    RSEM_REQUIRE(!m->est_rspd || ascending(m->r_cdf, (size_t)m->B + 1), "rsem_sim_create: r_cdf must be a finite running sum");
    if (q) {
        RSEM_REQUIRE(ascending(m->qc_init, kQ) && rows_ascending(m->qc_trans, kQ, kQ), "rsem_sim_create: qc_init and qc_trans must be finite running sums");
        RSEM_REQUIRE(rows_ascending(m->pc, (size_t)kQ * kCodes, kCodes) && rows_ascending(m->npc, kQ, kCodes), "rsem_sim_create: pc and npc must be finite running sums");
    } else {
        RSEM_REQUIRE(rows_ascending(m->pc, (size_t)m->pro_len * kCodes, kCodes) && ascending(m->npc, kCodes), "rsem_sim_create: pc and npc must be finite running sums");
    }
    const int max_len = m->has_mld ? m->m_ub : m->g_ub;

    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) {
        rsem::set_last_error("rsem_sim_create: no GPU %d", device);
        return RSEM_ERR_NODEVICE;
    }
    RSEM_HIP_TRY(hipSetDevice(device));
    rsem_sim* h = new rsem_sim();
    struct Guard { rsem_sim* h; ~Guard() { if (h) rsem_sim_destroy(h); } } guard{h};
    h->device = device;
    h->q_model = q;
    Tables& T = h->T;
    T.type = m->type; T.M = m->M; T.has_mld = m->has_mld ? 1 : 0; T.est_rspd = m->est_rspd ? 1 : 0; T.B = m->B; T.pro_len = q ? 0 : m->pro_len;
    T.g_lb = m->g_lb; T.g_ub = m->g_ub; T.m_lb = m->m_lb; T.m_ub = m->m_ub; T.prob_f = m->prob_f;
    T.plain = tables_plain(*m) ? 1 : 0;
    T.max_len = max_len;
    const size_t M1 = (size_t)m->M + 1;
    if (int rc = upload(h, &T.theta_cdf, m->theta_cdf, M1)) return rc;
    if (int rc = upload(h, &T.full_len, m->full_len, M1)) return rc;
    if (int rc = upload(h, &T.tot_len, m->tot_len, M1)) return rc;
    if (int rc = upload(h, &T.seq_off, m->seq_off, M1 + 1)) return rc;
    if (int rc = upload(h, &T.seq, m->seq, (size_t)m->seq_off[M1])) return rc;
    if (int rc = upload(h, &T.g_cdf, m->g_cdf, (size_t)(m->g_ub - m->g_lb) + 1)) return rc;
    if (m->has_mld)
        if (int rc = upload(h, &T.m_cdf, m->m_cdf, (size_t)(m->m_ub - m->m_lb) + 1)) return rc;
    if (m->est_rspd) {
        if (int rc = upload(h, &T.r_pdf, m->r_pdf, (size_t)m->B + 2)) return rc;
        if (int rc = upload(h, &T.r_cdf, m->r_cdf, (size_t)m->B + 2)) return rc;
    }
    if (q) {
        if (int rc = upload(h, &T.qc_init, m->qc_init, (size_t)kQ)) return rc;
        if (int rc = upload(h, &T.qc_trans, m->qc_trans, (size_t)kQ * kQ)) return rc;
        if (int rc = upload(h, &T.pc, m->pc, (size_t)kQ * 25)) return rc;
        if (int rc = upload(h, &T.npc, m->npc, (size_t)kQ * 5)) return rc;
    } else {
        if (int rc = upload(h, &T.pc, m->pc, (size_t)m->pro_len * 25)) return rc;
        if (int rc = upload(h, &T.npc, m->npc, (size_t)kCodes)) return rc;
    }
    RSEM_HIP_TRY(h->mem.alloc(&h->d_counts, M1 + 1));
    RSEM_HIP_TRY(hipMemset(h->d_counts, 0, (M1 + 1) * 8));
    RSEM_HIP_TRY(h->mem.alloc(&h->d_state, 1));
    RSEM_HIP_TRY(hipMemset(h->d_state, 0, sizeof(ChunkState)));
    RSEM_HIP_TRY(h->q.create());
    RSEM_HIP_TRY(hipEventCreate(&h->ed));
    if (q) {  // more dynamic LDS than the 64 KB a kernel gets unasked
        const int bytes = (int)(kLdsDoubles * sizeof(double));
        RSEM_HIP_TRY(hipFuncSetAttribute((const void*)k_sim_counter, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        RSEM_HIP_TRY(hipFuncSetAttribute((const void*)k_sim_heads, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        RSEM_HIP_TRY(hipFuncSetAttribute((const void*)k_sim_body, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    }
    h->device_bytes = h->mem.bytes;
    guard.h = nullptr;
    *out = h;
    return RSEM_OK;
}

extern "C" void rsem_sim_destroy(rsem_sim* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    for (Buf& b : h->buf) b.release(h->device_bytes);
    if (h->ed) (void)hipEventDestroy(h->ed);
    h->q.release();
    delete h;  // (the tables: DevMem)
}

extern "C" int rsem_sim_info(const rsem_sim* h, int32_t* max_len, int32_t* plain) {
    RSEM_REQUIRE(h, "rsem_sim_info: the handle must not be NULL");
    if (max_len) *max_len = h->T.max_len;
    if (plain) *plain = h->T.plain;
    return RSEM_OK;
}

extern "C" int rsem_sim_counter_batch(rsem_sim* h, uint64_t seed, uint64_t first_read, int64_t n_reads, rsem_sim_batch* b) {
    RSEM_REQUIRE(h, "rsem_sim_counter_batch: the handle must not be NULL");
    if (int rc = check_batch(h, b, n_reads, "rsem_sim_counter_batch")) return rc;
    rsem_sim_knobs k;
    if (int rc = read_knobs(&k)) return rc;
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->dead) { rsem::set_last_error("rsem_sim_counter_batch: a batch before this one ended with a status"); return RSEM_ERR_STATE; }
    clear_batch(b);
    b->device_bytes = h->device_bytes;
    if (n_reads == 0) return RSEM_OK;
    RSEM_HIP_TRY(hipSetDevice(h->device));
    Out o;
    if (int rc = device_out(h, n_reads, b->stride, o)) return rc;
    hipStream_t st = h->q.st;
    unsigned long long* d_resim = h->d_counts + (size_t)h->T.M + 1;
    // (a batch that ends with a status adds nothing: the counts are put back from a copy)
    std::vector<unsigned long long> before((size_t)h->T.M + 2);
    RSEM_HIP_TRY(hipMemcpyAsync(before.data(), h->d_counts, before.size() * 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemsetAsync(h->d_state, 0, sizeof(ChunkState), st));
    RSEM_HIP_TRY(h->q.upload_begin());
    RSEM_HIP_TRY(h->q.upload_end());
    hipLaunchKernelGGL(k_sim_counter, dim3(blocks256((uint64_t)n_reads)), dim3(256), lds_bytes(h, k), st, h->T, lds_bytes(h, k) ? 1 : 0, seed, first_read, n_reads,
                       (uint32_t)k.attempt_cap, o, h->d_counts, d_resim, &h->d_state->status);
    RSEM_HIP_TRY(h->q.kernels_end());
    ChunkState cs;
    unsigned long long resim_now = 0;
    RSEM_HIP_TRY(hipMemcpyAsync(&cs, h->d_state, sizeof(cs), hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipMemcpyAsync(&resim_now, d_resim, 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    RSEM_HIP_TRY(hipGetLastError());
    b->n_launches = 1;
    double up = 0;
    if (int rc = h->q.add_laps(up, b->body_ms)) return rc;
    if (cs.status != kOk) {
        b->status = cs.status;
        h->dead = true;
        RSEM_HIP_TRY(hipMemcpy(h->d_counts, before.data(), before.size() * 8, hipMemcpyHostToDevice));
        return RSEM_OK;
    }
    b->resimulations = resim_now - before[(size_t)h->T.M + 1];
    h->resimulations += b->resimulations;
    b->n_reads = n_reads;
    b->device_bytes = h->device_bytes;
    return download(h, o, n_reads, b);
}

extern "C" int rsem_sim_reference_begin(rsem_sim* h, uint32_t seed) {
    RSEM_REQUIRE(h, "rsem_sim_reference_begin: the handle must not be NULL");
    std::lock_guard<std::mutex> lock(h->mu);
    h->gen = rsemh::RefMt19937(seed);
    h->pending.clear();
    h->carry_fails = 0;
    h->begun = true;
    return RSEM_OK;
}

extern "C" int rsem_sim_reference_batch(rsem_sim* h, int64_t max_reads, rsem_sim_batch* b) {
    RSEM_REQUIRE(h, "rsem_sim_reference_batch: the handle must not be NULL");
    if (int rc = check_batch(h, b, max_reads, "rsem_sim_reference_batch")) return rc;
    rsem_sim_knobs k;
    if (int rc = read_knobs(&k)) return rc;
    std::lock_guard<std::mutex> lock(h->mu);
    if (h->dead) { rsem::set_last_error("rsem_sim_reference_batch: a batch before this one ended with a status"); return RSEM_ERR_STATE; }
    if (!h->begun) { rsem::set_last_error("rsem_sim_reference_batch: rsem_sim_reference_begin comes first"); return RSEM_ERR_STATE; }
    clear_batch(b);
    b->device_bytes = h->device_bytes;
    if (max_reads == 0) return RSEM_OK;
    RSEM_HIP_TRY(hipSetDevice(h->device));
    Out o;
    if (int rc = device_out(h, max_reads, b->stride, o)) return rc;
    hipStream_t st = h->q.st;
    const uint32_t longest = longest_attempt(h->T), tile = (uint32_t)k.tile, cap = (uint32_t)k.attempt_cap;
    const size_t lds = lds_bytes(h, k);
    std::vector<unsigned long long> before((size_t)h->T.M + 1);
    RSEM_HIP_TRY(hipMemcpyAsync(before.data(), h->d_counts, before.size() * 8, hipMemcpyDeviceToHost, st));
    RSEM_HIP_TRY(hipStreamSynchronize(st));
    auto fail = [&](int32_t status) -> int {
        b->status = status;
        b->n_reads = 0;
        h->dead = true;
        RSEM_HIP_TRY(hipMemcpy(h->d_counts, before.data(), before.size() * 8, hipMemcpyHostToDevice));
        if (status == kPastWords) {  // longest_attempt() leaves the room: not a property of the input
            rsem::set_last_error("rsem_sim_reference_batch: an attempt ran past the words of its chunk");
            return RSEM_ERR_STATE;
        }
        return RSEM_OK;
    };
    int64_t got = 0;
    uint64_t resim = 0;
    while (got < max_reads) {
        const int64_t want = max_reads - got;
        // positions searched: the chunk, or what `want` reads of the longest kind take where that is less
        const uint32_t n_pos = (uint32_t)std::min<uint64_t>(k.chunk_words, (uint64_t)want * longest);
        const uint32_t n_words = n_pos + longest, n_tiles = (n_pos + tile - 1) / tile;
        const double t0 = now_ms();
        if (h->pending.size() < n_words) {
            const size_t have = h->pending.size();
            h->pending.resize(n_words);
            for (size_t i = have; i < n_words; i++) h->pending[i] = h->gen.next();
        }
        b->words_ms += now_ms() - t0;
        size_t tmp = 0;
        RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)(n_pos + 1), st));
        const size_t need[B_TMP + 1] = {(size_t)n_words * 4, (size_t)n_pos * 4, (size_t)n_pos * 4, ((size_t)n_pos + 1) * 8, ((size_t)n_pos + 1) * 8, (size_t)n_tiles * 4,
                                        (size_t)want * 4, tmp};
        for (int i = 0; i <= B_TMP; i++) RSEM_HIP_TRY(h->buf[i].need(std::max<size_t>(need[i], 8), h->device_bytes));
        uint32_t* d_words = h->buf[B_WORDS].as<uint32_t>();
        uint32_t* d_next = h->buf[B_NEXT].as<uint32_t>();
        uint32_t* d_exit = h->buf[B_EXIT].as<uint32_t>();
        unsigned long long* d_flags = h->buf[B_FLAGS].as<unsigned long long>();
        unsigned long long* d_sums = h->buf[B_SUMS].as<unsigned long long>();
        uint32_t* d_entry = h->buf[B_ENTRY].as<uint32_t>();
        uint32_t* d_starts = h->buf[B_STARTS].as<uint32_t>();
        RSEM_HIP_TRY(hipMemsetAsync(h->d_state, 0, sizeof(ChunkState), st));
        RSEM_HIP_TRY(h->q.upload_begin());
        RSEM_HIP_TRY(hipMemcpyAsync(d_words, h->pending.data(), (size_t)n_words * 4, hipMemcpyHostToDevice, st));
        RSEM_HIP_TRY(h->q.upload_end());
        // (with plain tables the search draws no quality and no base: it leaves the tables where they are)
        const size_t lds_heads = h->T.plain ? 0 : lds;
        hipLaunchKernelGGL(k_sim_heads, dim3(blocks256(n_pos)), dim3(256), lds_heads, st, h->T, lds_heads ? 1 : 0, d_words, n_words, n_pos, d_next);
        hipLaunchKernelGGL(k_sim_tile_exits, dim3(n_tiles), dim3(kTileThreads), 0, st, d_next, n_pos, tile, d_exit, d_flags, d_entry);
        hipLaunchKernelGGL(k_sim_hop, dim3(1), dim3(64), 0, st, d_exit, n_pos, tile, d_entry, h->d_state);
        hipLaunchKernelGGL(k_sim_mark, dim3(n_tiles), dim3(kTileThreads), 0, st, d_next, n_pos, tile, d_entry, d_flags);
        size_t tb = h->buf[B_TMP].cap;
        RSEM_HIP_TRY(hipcub::DeviceScan::ExclusiveSum(h->buf[B_TMP].p, tb, d_flags, d_sums, (int)(n_pos + 1), st));
        hipLaunchKernelGGL(k_sim_starts, dim3(blocks256(n_pos)), dim3(256), 0, st, d_flags, d_sums, n_pos, (uint32_t)want, d_starts);
        RSEM_HIP_TRY(hipEventRecord(h->ed, st));
        unsigned long long totals = 0;
        ChunkState cs;
        RSEM_HIP_TRY(hipMemcpyAsync(&totals, d_sums + n_pos, 8, hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipMemcpyAsync(&cs, h->d_state, sizeof(cs), hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        b->n_launches += 6;
        b->n_chunks++;
        const uint64_t reads_seen = totals & 0xffffffffull, fails_seen = totals >> 32;
        const uint32_t n = (uint32_t)std::min<uint64_t>(reads_seen, (uint64_t)want);
        if (cs.exit_pos < n_pos || cs.exit_pos > n_words) { rsem::set_last_error("rsem_sim_reference_batch: a chunk of %u positions left at %u", n_pos, cs.exit_pos); return RSEM_ERR_STATE; }
        uint64_t consumed = cs.exit_pos;
        if (n) {
            hipLaunchKernelGGL(k_sim_body, dim3(blocks256(n)), dim3(256), lds, st, h->T, lds ? 1 : 0, d_words, n_words, d_starts, d_sums, n,
                               (uint32_t)std::min<uint64_t>(h->carry_fails, 0xffffffffull), cap, o, got, h->d_counts, h->d_state);
            b->n_launches += 1;
        }
        RSEM_HIP_TRY(h->q.kernels_end());
        RSEM_HIP_TRY(hipMemcpyAsync(&cs, h->d_state, sizeof(cs), hipMemcpyDeviceToHost, st));
        RSEM_HIP_TRY(hipStreamSynchronize(st));
        RSEM_HIP_TRY(hipGetLastError());
        float ms = 0;
        if (int rc = h->q.add_upload_lap(b->upload_ms)) return rc;
        RSEM_HIP_TRY(hipEventElapsedTime(&ms, h->q.eb, h->ed));
        b->search_ms += ms;
        RSEM_HIP_TRY(hipEventElapsedTime(&ms, h->ed, h->q.ec));
        b->body_ms += ms;
        if (cs.status != kOk) return fail(cs.status);
        // A failed attempt counts when a read claims it (simulation.cpp:122 counts inside a read's loop): those behind the last read taken
        // are carried, and a run that ends there never made them.
        if (n) {
            resim += h->carry_fails + cs.last_fails;
            if (reads_seen > n) {  // the batch is full inside the chunk: the stream goes on behind its last read
                consumed = cs.last_next;
                h->carry_fails = 0;
            } else h->carry_fails = fails_seen - cs.last_fails;
        } else h->carry_fails += fails_seen;
        if (h->carry_fails >= cap) return fail(kAttemptCap);
        if (consumed == 0 || consumed > n_words) { rsem::set_last_error("rsem_sim_reference_batch: %llu words consumed of %u", (unsigned long long)consumed, n_words); return RSEM_ERR_STATE; }
        h->pending.erase(h->pending.begin(), h->pending.begin() + (size_t)consumed);
        b->stream_words += consumed;
        got += n;
    }
    b->n_reads = got;
    b->resimulations = resim;
    h->resimulations += resim;
    b->device_bytes = h->device_bytes;
    return download(h, o, got, b);
}

extern "C" int rsem_sim_totals(rsem_sim* h, uint64_t* counts, uint64_t* resimulations) {
    RSEM_REQUIRE(h, "rsem_sim_totals: the handle must not be NULL");
    RSEM_REQUIRE(counts, "rsem_sim_totals: counts must not be NULL");
    std::lock_guard<std::mutex> lock(h->mu);
    RSEM_HIP_TRY(hipSetDevice(h->device));
    RSEM_HIP_TRY(hipMemcpy(counts, h->d_counts, ((size_t)h->T.M + 1) * 8, hipMemcpyDeviceToHost));
    if (resimulations) *resimulations = h->resimulations;
    return RSEM_OK;
}
