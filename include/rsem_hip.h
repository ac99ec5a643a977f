/* rsem_hip.h -- C ABI of librsem_hip.so: RSEM's EM / Gibbs hot path on MI355X (gfx950).
 *
 * The reference (deweylab/RSEM) has no FFI: its hot path is reached through two executables,
 * rsem-run-em (EM.cpp) and rsem-run-gibbs (Gibbs.cpp), whose in-process seams are the pthread
 * entry points  E_STEP<>(Params{model,reader,hitv,ncpv,mhp,countv})  (EM.cpp:57-60,176-247) and
 * Gibbs(Params{no,nsamples,fo,engine,pme_c,...})  (Gibbs.cpp:29-37,265-353): a CSR shard in,
 * per-shard count vector / per-chain accumulators out.  Each entry point below replaces one of
 * those seams (cited per function).  Conventions:
 *   - plain C types; host pointers are caller-owned and only read/written during the call;
 *   - an opaque ctx owns all device memory of one GPU; calls on one ctx are serialised by the caller;
 *   - every function returns RSEM_OK (0) or a negative rsem_status; rsem_hip_strerror() explains,
 *     rsem_hip_last_error() gives the HIP detail of the calling thread's last failure;
 *   - no exceptions, no exit() across the boundary (the reference exits on error, my_assert.h:89-96;
 *     the CLI wrappers in rsem_amd/csrc/host keep that behaviour on top of these codes);
 *   - there is NO CPU fallback: without a usable gfx950 device every *_create fails with
 *     RSEM_ERR_NODEVICE.
 */
#ifndef RSEM_HIP_H_
#define RSEM_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RSEM_OK = 0,
    RSEM_ERR_INVALID = -1,  /* bad argument (NULL, sid out of range, non-monotone row_ptr, ...) */
    RSEM_ERR_HIP = -2,      /* a HIP runtime call failed; see rsem_hip_last_error() */
    RSEM_ERR_NOMEM = -3,    /* device or host allocation failed */
    RSEM_ERR_NODEVICE = -4, /* no such GPU / not a gfx950-class device */
    RSEM_ERR_STATE = -5     /* call sequence error (e.g. values never set) */
} rsem_status;

const char* rsem_hip_strerror(int status);
const char* rsem_hip_last_error(void);
int rsem_hip_device_count(int* n);
/* Properties of a device the host programs size their decisions by: key = "compute_units" | "clock_khz" | "hbm_bytes". */
int rsem_hip_device_info(int device, const char* key, int64_t* value);
/* Initialise the HIP runtime and the device context (callable from a helper thread while inputs are parsed). */
int rsem_hip_warmup(int device);
/* ... and load the device code of the parts a program is going to use, so that the first real launch does not pay for it
 * (the runtime loads a translation unit's code object at its first launch: tens of milliseconds each).  what = OR of: */
#define RSEM_PRELOAD_EM 1
#define RSEM_PRELOAD_MODEL 2
#define RSEM_PRELOAD_GIBBS 4
#define RSEM_PRELOAD_CI 8
int rsem_hip_preload(int device, int what);
/* ABI version of this header: bumped on any signature change. */
int rsem_hip_abi_version(void);
/* Measurement aid ("also measure a device STREAM-copy and report both"): streams `bytes` of HBM
 * `reps` times with 16-byte-per-lane non-temporal wave loads, eight in flight per lane, and reports the best rate seen, in GB/s
 * (1e9 bytes per second; copy counts bytes read + bytes written).  Nothing of the hot path depends on it. */
int rsem_hip_stream_probe(int device, uint64_t bytes, int reps, double* read_GBps, double* copy_GBps);

/* ------------------------------------------------------------------------------------------
 * Communicators of the multi-GPU paths.  The reference's parallelism is pthreads over one address
 * space: its "collectives" are the serial sums countvs[0][j] += countvs[i][j] (EM.cpp:385-389) and
 * pme_c[j] += params[i].pme_c[j] (Gibbs.cpp:372-388).  With the shards / chains on different GPUs
 * those sums are RCCL collectives enqueued on the ctx stream.  One rank per GPU; the ranks may be
 * threads of one process (the CLI programs) or one process each (bench.py: the id travels through
 * torch.distributed).
 * ------------------------------------------------------------------------------------------ */
typedef struct rsem_comm rsem_comm;
#define RSEM_COMM_ID_BYTES 128
/* ncclGetUniqueId: call on one rank, hand the bytes to all the others. */
int rsem_comm_unique_id(char* id /* RSEM_COMM_ID_BYTES */);
/* ncclCommInitRank on `device`; collective over all `world` ranks (call concurrently). */
int rsem_comm_create(rsem_comm** out, int device, int rank, int world, const char* id);
/* A group of `world` ranks inside one process that may share devices (RCCL refuses two ranks on one GPU): the
 * exchange goes through the ranks' device buffers with host barriers.  For exercising the sharded paths on a
 * single-GPU machine; out[world]. */
int rsem_comm_create_local(rsem_comm** out, int world, const int* devices);
int rsem_comm_rank(const rsem_comm* comm);
int rsem_comm_world(const rsem_comm* comm);
/* In-place sum of n doubles at device pointer d_buf over all ranks, ordered on `stream` (tests / tools). */
int rsem_comm_allreduce_f64(rsem_comm* comm, void* d_buf, uint64_t n, void* stream);
int rsem_comm_destroy(rsem_comm* comm);

/* ------------------------------------------------------------------------------------------
 * EM (rsem-run-em).  Replaces: HitContainer<HitType> (HitContainer.h:12-59, SingleHit.h:8-51),
 * init<> sharding (EM.cpp:97-174), E_STEP<> (EM.cpp:176-247) and the count reduction / M step /
 * convergence test of EM<> (EM.cpp:383-416).
 * ------------------------------------------------------------------------------------------ */
typedef struct rsem_em_ctx rsem_em_ctx;

/* E-step kernel variants (rsem_em_set_option "kernel") */
#define RSEM_EM_KERNEL_AUTO 0
#define RSEM_EM_KERNEL_CSR 1   /* RETIRED in round 6 (was: thread-per-read over the CSR as given); rsem_em_set_option refuses it */
#define RSEM_EM_KERNEL_SELL 2  /* RETIRED in round 6 (was: per-slice segmented shuffle reduction, a cross-check); refused */
#define RSEM_EM_KERNEL_LANE 3  /* sliced layout, lane-private runs, LDS-staged theta + LDS count window (default) */

/* Upload one shard: N1 reads, nnz alignments.  row_ptr[N1+1] (row_ptr[0]==0, row_ptr[N1]==nnz),
 * sid[nnz] in 1..M (strand already stripped: HitType::getSid, SingleHit.h:26),
 * conprb[nnz] / ncp[N1] may be NULL when they will be supplied by rsem_em_set_values or computed
 * on the device by the rsem_model_* entry points.  (HitContainer::read, HitContainer.h:63-79.) */
int rsem_em_create(rsem_em_ctx** out, int device, int32_t M, uint64_t N1, uint64_t nnz,
                   const uint64_t* row_ptr, const int32_t* sid, const double* conprb,
                   const double* ncp);
/* Replace the CSR values (hit.setConPrb / ncpv[i], EM.cpp:210,216) in the caller's (file) order. */
int rsem_em_set_values(rsem_em_ctx* ctx, const double* conprb, const double* ncp);
/* The current values in caller order (conprb[nnz], ncp[N1]) -- what rsem_em_create / rsem_em_set_values put there or the model
 * rounds computed (hit.getConPrb() / ncpvecs of EM.cpp:421-458 when it writes imdName.ofg).  Works after option "release_csr"
 * (the values are read back from the planes first). */
int rsem_em_get_values(rsem_em_ctx* ctx, double* conprb, double* ncp);
/* Options (none of them is part of the reference's surface):
 *   "kernel"            RSEM_EM_KERNEL_AUTO or _LANE (the cross-check variants were retired in round 6);
 *   "split_rows"        1 (default) / 0: reads with transcript ids outside the LDS window of their own gene are laid out as a row of
 *                       their in-window alignments plus far entries handled by two passes around the E-step kernel;
 *   "split_policy"      1 (default): the reads that are MOSTLY outside split; 2: every read with an id outside (its split rows then
 *                       run on a stream of their own beside the compact reads: "split_overlap" 1, the default with policy 2) --
 *                       measured equal or slower on the bench's inputs, kept as an option;
 *   "check_every"       rounds between the host's looks at the loop;
 *   "value_bits"        64 (default): the theta-only E step streams the conprb doubles as given; 32: reads whose
 *                       non-zero conprb values span less than 2^value_range_bits are streamed as 32-bit mantissas with
 *                       one exponent per read (value = m * 2^e, rounded to nearest: relative error <= 2^-33 of the
 *                       read's largest value), all other reads stay doubles.  Affects the counts of rsem_em_step /
 *                       rsem_em_run / rsem_em_expected_weights; the weights w[] always come from the doubles.
 *   "value_range_bits"  0..24, default 8;
 *   "release_csr"       1: free the caller-order transcript ids and values on the device (12 bytes per alignment: half of the
 *                       context's memory) -- the theta-only rounds of rsem_em_step / rsem_em_run stream the sliced layout
 *                       alone -- until something needs them again (weights, new values, a rebuild of the layout, a model
 *                       context), which reads them back from the planes: the same doubles.  RSEM_ERR_STATE, nothing changed,
 *                       where the planes do not hold everything (Q32 planes, split rows, reads with more than 256
 *                       alignments, a live model context).  0: bring them back now. */
int rsem_em_set_option(rsem_em_ctx* ctx, const char* key, int64_t value);
/* Layout facts: "value_bits", "value_range_bits", "reads_q32", "reads_sliced", "reads_long", "value_plane_bytes",
 * "sid_plane_bytes", "slots", "units", "csr_released" (0 / 1), "csr_bytes" (what "release_csr" frees).
 * How the E step deals the units of the sliced layout to its launches, in their order:
 *   "units_compact"      units [0, units_compact) take no far-queue launch: the compact units, or all main units where the far
 *                        queue is not used;
 *   "units_main"         units [units_compact, units_main) take the far-queue launch; [units_main, units) are split rows;
 *   "units_queued"       main units that qualify for the far-queue launch (a few ids outside their window per slice), whether or
 *                        not it is taken (it is where they are at least one main unit in 25 and the far queue is on);
 *   "unit_tables_agree"  1 if the device copy of the unit table holds the same units in the same order as the host copy, else 0
 *                        (a diagnostic: it reads the table back). */
int rsem_em_get_info(const rsem_em_ctx* ctx, const char* key, int64_t* value);
/* Tuning aid (not part of the reference's surface): one E-step launch of the LANE kernel with per-workgroup start/end
 * timestamps (100 MHz clock), out[2u], out[2u+1] in dispatch order; *n_units_io = capacity in, units written out. */
int rsem_em_debug_trace(rsem_em_ctx* ctx, const double* theta, unsigned long long* out, uint32_t* n_units_io);
/* Diagnostic (not part of the reference's surface; it changes nothing in the context): the far entries of the split rows as the
 * two passes around the E-step kernel read them.  Row order: the entries of the split read in row slot x_slot_base + xs are
 * [far_ptr[xs], far_ptr[xs + 1]), xs < n_x_slots (empty slots included), in file order; far_sid[e] is an entry's transcript id,
 * far_src[e] its index into the caller's sid / conprb arrays.  Column order: the same entries sorted by (block of row slots,
 * transcript id), each with its id, the row slot of its read and its caller index (csc_sid / csc_slot / csc_src).
 * Two calls: with all six arrays NULL the sizes alone are written (*n_x_slots_io, *n_far_io; all 0 without split rows); with
 * all six given, *n_x_slots_io and *n_far_io say what the arrays hold (far_ptr one more) and come back as what was written. */
int rsem_em_debug_far(rsem_em_ctx* ctx, uint32_t* x_slot_base, uint32_t* n_x_slots_io, uint64_t* n_far_io, uint64_t* far_ptr,
                      int32_t* far_sid, uint64_t* far_src, int32_t* csc_sid, uint32_t* csc_slot, uint64_t* csc_src);
int rsem_em_destroy(rsem_em_ctx* ctx);

/* One E step + M step: round 1 of 1 of rsem_em_run's kernel sequence, over this context's reads alone (no all-reduce).
 * theta[M+1] in; counts[M+1] out = fractional counts incl. +N0 in bin 0 (EM.cpp:385-392), theta_new = counts / (N0 + the
 * number of reads with a non-zero normaliser) -- the exact value of the sum the reference divides by (EM.cpp:394-398) --,
 * sum = the floating-point sum of the counts (the SUM of the reference's ROUND line), and the convergence statistics
 * bChange / totNum (EM.cpp:406-413).  Any output pointer may be NULL. */
int rsem_em_step(rsem_em_ctx* ctx, const double* theta, double N0, double* counts,
                 double* theta_new, double* sum, double* bChange, int32_t* totNum);

/* Per-run measurements filled by rsem_em_run when non-NULL (HIP events on the ctx stream). */
typedef struct {
    double total_ms;        /* first E-step launch .. last M-step kernel of the run */
    double estep_ms_sum;    /* sum of per-launch E-step kernel durations */
    int32_t estep_launches; /* number of E-step launches timed */
    int32_t rounds;         /* rounds executed */
    uint64_t algorithmic_bytes_per_round; /* 12*nnz + 16*N1 + 16*(M+1), SURVEY.md section 8(d) */
} rsem_em_profile;

/* Device-resident EM loop for the rounds where the CSR values are frozen (ROUND >= 12 in the
 * reference, EM.cpp:365-416 with needCalcConPrb == updateModel == false): rounds round0+1, ... until
 * (ROUND >= min_round && totNum == 0) || ROUND == max_round.  theta_inout[M+1]; counts[M+1] (last
 * round's counts, may be NULL); rounds_done = last ROUND; bChange/totNum of that round. */
int rsem_em_run(rsem_em_ctx* ctx, double* theta_inout, double N0, int round0, int min_round,
                int max_round, int* rounds_done, double* counts, double* bChange, int32_t* totNum,
                rsem_em_profile* profile);

/* The line the reference prints after every round (EM.cpp:415): ROUND, SUM, bChange, totNum.  When set, rsem_em_run
 * calls fn on the calling thread for every round it executes, in order, shortly after the round finished on the
 * device (the loop itself never waits for the host).  fn = NULL switches it off. */
typedef void (*rsem_em_progress_fn)(int round, double sum, double bChange, int totNum, void* user);
int rsem_em_set_progress(rsem_em_ctx* ctx, rsem_em_progress_fn fn, void* user);

/* Rows sharded over the ranks of `comm` (the reference's thread split, EM.cpp:135-157): every
 * rank holds a ctx over its own reads and the same M; rsem_em_run then must be called on all ranks with the same
 * theta, the GLOBAL N0 and the same round arguments, and sums the fractional counts of every round over the ranks
 * with one all-reduce of M+1 (+ a few) doubles on the ctx stream (EM.cpp:385-389) before the M step, which every
 * rank computes identically.  comm is not owned; NULL detaches. */
int rsem_em_set_comm(rsem_em_ctx* ctx, rsem_comm* comm);
/* The reference's split of the reads over T workers (EM.cpp:135-157): worker i takes rows until it holds >= nHits / T
 * alignments, the last one the rest, every later worker at least one row.  Host-only; bounds[world + 1]. */
int rsem_em_shard_rows(uint64_t N1, const uint64_t* row_ptr, int world, uint64_t* bounds);

/* Final pass with calcExpectedWeights = true (EM.cpp:460-478): counts incl. +N0, posterior weight
 * of every alignment w[nnz] (file order) and of the noise transcript w_noise[N1]; rows whose
 * normaliser is < 1e-300 get zeros (EM.cpp:237-243). */
int rsem_em_expected_weights(rsem_em_ctx* ctx, const double* theta, double N0, double* counts,
                             double* w, double* w_noise);

/* ------------------------------------------------------------------------------------------
 * Read models (rounds 1-11 of rsem-run-em).  Replaces the per-read / per-alignment work of
 * SingleModel / SingleQModel / PairedEndModel / PairedEndQModel: getConPrb + getNoiseConPrb
 * (SingleQModel.h:101-162, PairedEndQModel.h:94-155 and the no-quality twins) as used by
 * E_STEP<> when needCalcConPrb (EM.cpp:210,216) and calcConProbs (EM.cpp:249-278), and
 * update + updateNoise (SingleQModel.h:168-221, PairedEndQModel.h:161-188) when updateModel
 * (EM.cpp:226,233).  The O(table) work between rounds (init / collect / finish / calcMW) stays
 * with the caller (rsem_amd/csrc/host/model_host.hpp).
 * ------------------------------------------------------------------------------------------ */
typedef struct rsem_model_ctx rsem_model_ctx;

/* Immutable inputs, all in the order of imd.dat / imd_alignable*.f[aq] (host pointers, copied). */
typedef struct {
    int32_t model_type;          /* 0 Single, 1 SingleQ, 2 PairedEnd, 3 PairedEndQ */
    int32_t M;
    uint64_t N1, nnz;
    const uint64_t* row_ptr;     /* [N1+1] */
    const int32_t* sid_signed;   /* [nnz] as in .dat: negative = reverse strand (SingleHit.h:24-26) */
    const int32_t* pos;          /* [nnz] */
    const int32_t* insertL;      /* [nnz], paired-end only (PairedEndHit.h:8-34), else NULL */
    /* reads: base ids 0..4 = A C G T N (utils.h:36-50), quality = ASCII - 33 (QProfile.h:44); mate 2 NULL for SE */
    const uint64_t* read_off[2]; /* [N1+1] offsets into read_seq / read_qual */
    const uint8_t* read_seq[2];
    const uint8_t* read_qual[2]; /* NULL for the no-quality models */
    const uint8_t* low_quality;  /* [N1] Read::isLowQuality() after calc_lq (SingleReadQ.h:63-95, PairedEndReadQ.h:55-62) */
    /* references (RefSeq.h): forward-strand base ids incl. poly(A) tail, concatenated */
    const uint64_t* ref_off;     /* [M+2], ref_off[0] = ref_off[1] = 0 */
    const uint8_t* ref_seq;
    const int32_t* fullLen;      /* [M+1] */
    const int32_t* totLen;       /* [M+1] */
    const uint64_t* mask_off;    /* [M+2] offsets (in 32-bit words) into mask_words */
    const uint32_t* mask_words;  /* RefSeq::fmasks */
} rsem_model_data;

/* The current model parameters (one EM round's view of the master model). */
typedef struct {
    double probF;                /* Orientation */
    int32_t seedLen;
    int32_t estRSPD, B;          /* RSPD: pdf/cdf [B+2] */
    const double* rspd_pdf;
    const double* rspd_cdf;
    int32_t gld_lb, gld_ub;      /* LenDist gld: pdf/cdf [ub-lb+1] */
    const double* gld_pdf;
    const double* gld_cdf;
    int32_t has_mld, mld_lb, mld_ub;
    const double* mld_pdf;
    const double* mld_cdf;
    int32_t prof_rows;           /* 100 (QProfile) or proLen (Profile) */
    const double* prof;          /* [prof_rows*25]  p[q or i][ref][read] */
    const double* noise;         /* [100*5] NoiseQProfile p, or [5] NoiseProfile p */
    const double* mw;            /* [M+1] */
} rsem_model_tables;

/* Sums accumulated by one rsem_model_estep_update (the merged helper models of EM.cpp:400-404). */
typedef struct {
    double* prof;                /* [prof_rows*25] */
    double* noise;               /* [100*5] or [5] */
    double* rspd;                /* [B+2] (estRSPD only, else may be NULL) */
    double* gld;                 /* [gld0_ub-gld0_lb+1] over the ORIGINAL support (paired-end only, else NULL) */
    int32_t gld0_lb, gld0_ub;    /* in: support of the helper models' gld (mparams minL-1, maxL) */
} rsem_model_accum;

/* `em` must have been created with the same CSR (|sid_signed|); the model ctx writes the CSR values of
 * `em` on the device and drives its E step. */
int rsem_model_create(rsem_model_ctx** out, rsem_em_ctx* em, const rsem_model_data* data);
int rsem_model_set_tables(rsem_model_ctx* ctx, const rsem_model_tables* t);
/* conprb of every alignment and the noise conprb of every read with the current tables -> em values */
int rsem_model_calc_conprb(rsem_model_ctx* ctx);
/* One round with updateModel = true (EM.cpp:199-236): E step, counts/theta_new/statistics as
 * rsem_em_step, plus the model sufficient statistics weighted by the posterior fractions. */
int rsem_model_estep_update(rsem_model_ctx* ctx, const double* theta, double N0, double* counts,
                            double* theta_new, double* sum, double* bChange, int32_t* totNum,
                            rsem_model_accum* acc);
/* One whole model round (EM.cpp:199-236 with needCalcConPrb = true; updateModel = (acc != NULL)) in ONE pass over the
 * reads: P(read, alignment | transcript) from the tables last set (SingleQModel.h:101-162, PairedEndQModel.h:94-155 and
 * twins), the posterior weights for `theta` (EM.cpp:227,234) and, when `acc` is given, the model's sufficient statistics
 * (SingleQModel.h:168-221, PairedEndQModel.h:161-188); outputs as rsem_em_step.  Equivalent to rsem_model_calc_conprb
 * followed by rsem_model_estep_update (acc != NULL) or rsem_em_step (acc == NULL). */
int rsem_model_round(rsem_model_ctx* ctx, const double* theta, double N0, double* counts, double* theta_new,
                     double* sum, double* bChange, int32_t* totNum, rsem_model_accum* acc /* NULL: no statistics */);
/* current CSR values back to the host in file order (for imd.ofg, EM.cpp:421-457) */
int rsem_model_get_values(rsem_model_ctx* ctx, double* conprb, double* ncp);
/* Facts of a model context:
 *   "window_addr_bits"  the width of the per-alignment addresses into the array of transcript strands: 32 while both strands of
 *                       every transcript (each rounded up to 8 bytes) + 16 bytes stay below 2^32, else 40.  References beyond
 *                       2^40 bytes are refused by rsem_model_create (RSEM_ERR_INVALID), before anything is uploaded;
 *   "strand_bytes"      both strands of every transcript, each rounded up to 8 bytes;
 *   "strand_pad_bytes"  the environment variable RSEM_MODEL_STRAND_PAD, read by rsem_model_create (a whole number of bytes, a
 *                       multiple of 8; anything else makes the create fail with RSEM_ERR_INVALID): device bytes allocated in front
 *                       of the strands, never written or read, counted in every address (a test knob: small inputs above 2^32). */
int rsem_model_get_info(const rsem_model_ctx* ctx, const char* key, int64_t* value);
int rsem_model_destroy(rsem_model_ctx* ctx);

/* ------------------------------------------------------------------------------------------
 * Gibbs (rsem-run-gibbs).  Replaces: Item / s / hits (Gibbs.cpp:39-47,63-64), Gibbs()
 * (Gibbs.cpp:265-353) incl. sample() (sampling.h:50-65), and the per-chain accumulators that
 * release() sums (Gibbs.cpp:355-388).
 * ------------------------------------------------------------------------------------------ */
typedef struct rsem_gibbs_ctx rsem_gibbs_ctx;

#define RSEM_GIBBS_EXACT 0    /* the reference's sequential collapsed chain, MT19937, bit-identical draws */
#define RSEM_GIBBS_PARALLEL 1 /* data-augmentation sampler (theta | z, then z | theta in parallel), Philox */

/* items CSR incl. the noise column (sid 0), as in .ofg (EM.cpp:435-457).  init_counts[M+1] is 0 or
 * -1 (omitted transcripts, Gibbs.cpp:152-167); alpha[M+1] or NULL (scalar pseudoC); eel/mw[M+1];
 * grp[m+1] gene start indices (GroupInfo.h:34-53). */
int rsem_gibbs_create(rsem_gibbs_ctx** out, int device, int32_t M, uint64_t N1, uint64_t nitems,
                      const uint64_t* row_ptr, const int32_t* sid, const double* conprb,
                      const int32_t* init_counts, const double* alpha, double pseudoC, double totc,
                      uint64_t N0, const double* eel, const double* mw, int32_t m, const int32_t* grp);
/* Per-run measurements filled by rsem_gibbs_run_chains when non-NULL (HIP events on the ctx stream). */
typedef struct {
    double total_ms;   /* first sweep .. last per-sample statistics kernel */
    double sweep_ms;   /* total_ms / sweeps */
    int64_t sweeps;    /* EXACT: rounds (every chain advances in each); PARALLEL: z passes summed over the chains */
    int32_t chains;
    int32_t team;      /* EXACT: workgroups per chain (k_gibbs_exact_team; 1 = one workgroup per chain); 0 otherwise.  (Sits in what
                        * was padding: the layout of the other fields is unchanged.) */
    double reduce_ms;  /* the ONE collective of the multi-GPU split (reduce of the chain sums to rank 0), 0 without a communicator */
} rsem_gibbs_profile;

/* Run nchains independent chains on this GPU -- the reference's worker threads (Gibbs.cpp:207-254): chain k starts
 * from MT19937(seeds[k]) (EXACT) / Philox keyed by seeds[k] (PARALLEL), keeps nsamples[k] samples after `burnin`
 * rounds, one every `gap` rounds.  EXACT: a team of workgroups per chain, all chains in every launch.  PARALLEL: one chain after
 * the other (a sweep fills the GPU).  count_vectors: NULL, or nchains host pointers (each NULL or nsamples[k] x (M+1)
 * int32 = the lines of imd.countvectors<k>, Gibbs.cpp:257-262).  The accumulators receive the SUMS over the kept
 * samples of all chains, added in chain order (release(), Gibbs.cpp:372-388; not yet divided): pme_c, pve_c (sum of
 * squares), pme_tpm, pme_fpkm [M+1], pve_c_genes [m], pve_c_trans [m_trans] (NULL unless allele groups are set).
 * With rsem_gibbs_set_comm the sums are additionally reduced over the communicator and valid on rank 0 only. */
int rsem_gibbs_run_chains(rsem_gibbs_ctx* ctx, int mode, int nchains, const uint32_t* seeds, int burnin,
                          const int32_t* nsamples, int gap, int thin /* PARALLEL only: z passes per round, >= 1 */,
                          int32_t* const* count_vectors, double* pme_c, double* pve_c, double* pme_tpm,
                          double* pme_fpkm, double* pve_c_genes, double* pve_c_trans, rsem_gibbs_profile* prof);
/* One chain: rsem_gibbs_run_chains with nchains = 1 (sweep_ms may be NULL). */
int rsem_gibbs_run(rsem_gibbs_ctx* ctx, int mode, uint32_t seed, int burnin, int nsamples, int gap,
                   int thin, int32_t* count_vectors, double* pme_c, double* pve_c, double* pme_tpm,
                   double* pme_fpkm, double* pve_c_genes, double* sweep_ms /* may be NULL */);
/* Allele-specific references (ref.ta, GroupInfo.h): ta[m_trans+1] = first allele of every transcript.  After this
 * call every rsem_gibbs_run also accumulates, per kept sample, the squared per-transcript count sums
 * (pve_c_trans, Gibbs.cpp:339-345); rsem_gibbs_get_pve_c_trans returns the last run's sums [m_trans].  ta, as grp of
 * rsem_gibbs_create, must start at 1, end at M+1 and never decrease (RSEM_ERR_INVALID, nothing changed). */
int rsem_gibbs_set_allele_groups(rsem_gibbs_ctx* ctx, int32_t m_trans, const int32_t* ta);
int rsem_gibbs_get_pve_c_trans(rsem_gibbs_ctx* ctx, double* pve_c_trans);
/* Chains sharded over GPUs: every later rsem_gibbs_run_chains ends with ONE reduce of its
 * accumulator sums to rank 0 of `comm` (RCCL over xGMI), replacing the host loop of release() (Gibbs.cpp:372-388).
 * Count vectors need no communication: a rank writes the files of its own chains.  comm is not owned; NULL detaches. */
int rsem_gibbs_set_comm(rsem_gibbs_ctx* ctx, rsem_comm* comm);
/* Test aid (not part of the reference's surface; reads only): the read order of the PARALLEL sampler's layout, built now
 * if it is not yet.  The sampler keys a read's random number by its position in that order.  order[p] = the caller's read
 * at sorted position p, lg[p] = log2 of the lanes that read takes in the sliced layout (0..6), or RSEM_GIBBS_ORDER_LONG for
 * the reads that stay in the CSR (more than 256 non-noise items: positions n_sell_rows .. N1-1).  order, lg: N1 entries. */
#define RSEM_GIBBS_ORDER_LONG 255
int rsem_gibbs_debug_order(rsem_gibbs_ctx* ctx, uint32_t* order, uint8_t* lg, uint32_t* n_sell_rows);
/* ... and how the sweep kernel walks it (reads only): *T = slices per block; *n_units_io = capacity of `out` in, units of the
 * layout out; out (may be NULL: count only) takes 6 words per unit = one workgroup: first slice within its shape, slices,
 * slices per wave (wave w walks [first + w * per_wave, + per_wave), cut at the unit's end; block b of a shape = its slices
 * [b * T, b * T + T)), 1 if an id of the unit lies outside its LDS window (the kernel's far path), lg and K of the shape.
 * The environment variable RSEM_GIBBS_LAYOUT_T (a whole number in 4..256; anything else makes building the layout fail with
 * RSEM_ERR_INVALID), read when the layout is built, sets T (a measurement / test knob). */
int rsem_gibbs_debug_units(rsem_gibbs_ctx* ctx, uint32_t* T, uint32_t* n_units_io, uint32_t* out);
/* ... and the LDS window of every unit, in the same order (reads only): 2 words per unit, the first id of the window and the ids
 * it holds.  An anchor id above 2^23 - 1 is kept as 2^23 - 1 (sell_layout.hpp kKeyMinSidCap): a unit of such reads alone has its
 * window there, one id wide where none of its ids comes that far down, and takes the far path. */
int rsem_gibbs_debug_unit_windows(rsem_gibbs_ctx* ctx, uint32_t* n_units_io, int32_t* out);
int rsem_gibbs_destroy(rsem_gibbs_ctx* ctx);
/* sampling.h:19-44: seeds of the first nchains chains for --seed seed. */
int rsem_gibbs_chain_seeds(uint32_t seed, int nchains, uint32_t* out);

/* Convergence diagnostics of a run's count vectors (no counterpart in the reference, which writes the vectors, Gibbs.cpp:257-262,
 * and says nothing about whether its chains agree).  count_vectors: nchains host pointers, block k =
 * nsamples[k] x (M+1) int32 as rsem_gibbs_run_chains returns them = the lines of imd.countvectors<k>.  Every chain gives its LAST
 * n' = 2 * (min_k nsamples[k] / 2) rows, cut in two: m = 2 * nchains sequences of n = n' / 2 values per transcript.  Per transcript
 * 0 .. M: mean, sd = sqrt(var+), split-R-hat = sqrt(var+ / W), the effective sample size m n / tau with tau from Geyer's initial
 * monotone sequence over the autocorrelations (held at 1 / log10(m n) from below) and the last lag that sum took.  W = 0 gives
 * rhat = +inf (the sequences' means differ) or NaN (they do not), ess = NaN, lag = 0.  Needs no context; n < 2, NULL or negative
 * arguments: RSEM_ERR_INVALID; vectors that do not fit the device's free memory: RSEM_ERR_NOMEM, nothing attempted.
 * The environment variable RSEM_GIBBS_DIAG_L0 (odd, 1 .. 63; anything else: RSEM_ERR_INVALID), read at call time, sets the lag up
 * to which the first kernel decides a transcript (a test / measurement knob: the results do not depend on it, n_long does). */
typedef struct {
    int32_t n_used, sequences;  /* n' and m */
    int32_t n_defined;          /* ids 1 .. M (as everything below) with a finite rhat */
    int32_t max_rhat_id, min_ess_id;          /* smallest id among equals; 0: there is none */
    int32_t n_rhat_gt_1p01, n_rhat_gt_1p1;   /* +inf counts */
    int32_t n_long;             /* transcripts whose lag exceeds L0: finished by the one-wave-per-transcript kernel */
    double max_rhat, min_ess;   /* over the finite rhat / over the ess that are not NaN; NaN: there is none */
    double upload_ms, kernel_ms;
} rsem_gibbs_diag_summary;
int rsem_gibbs_diagnose(int device, int32_t M, int nchains, const int32_t* nsamples, const int32_t* const* count_vectors,
                        double* mean, double* sd, double* rhat, double* ess, int32_t* lag /* [M+1] each, any may be NULL */,
                        rsem_gibbs_diag_summary* summary /* may be NULL */);

/* ---- credibility intervals (rsem-calculate-credibility-intervals) -----------------------------------------
 * Replaces sample_theta_from_c + Buffer (calcCI.cpp:93-164, Buffer.h:13-80) and calcCI / calcCI_batch
 * (calcCI.cpp:216-388): for every Gibbs count vector, nSpC Dirichlet draws theta ~ Dir(c + pseudoC) / mw,
 * TPM samples (float) and the mean effective length l_bar per draw; then per transcript / gene the shortest
 * interval holding `confidence` of the samples and the coefficient of quartile variation, for TPM and FPKM.
 * The gamma variates come from a counter-based generator (Philox4x32-10 keyed by `seed`), not from the
 * reference's per-thread MT19937 streams: same distribution, different draws (the reference's own output
 * depends on -p).  The interval arithmetic on a given sample row is bit-identical to the reference's. */
typedef struct rsem_ci_profile {
    double sample_ms, sort_ms, interval_ms, total_ms;
    uint64_t n_draws, n_keys_sorted;
} rsem_ci_profile;

/* cvecs: nCV x (M+1) int32 count vectors (imd.countvectors*, Gibbs.cpp:257-262), row-major, index 0 = noise.
 * eel, mw: M+1.  gene_starts: m+1 (ref.grp).  trans_starts: m_trans+1 (ref.ta) or NULL when not allele-specific.
 * Outputs, each 3 x n floats laid out [lb[n] | ub[n] | cqv[n]]: tpm_ci / fpkm_ci n = M (sid 1..M),
 * gene_*_ci n = m, iso_*_ci n = m_trans (NULL when trans_starts is NULL). */
int rsem_ci_calculate(int device, int32_t M, int32_t nCV, int32_t nSpC, const int32_t* cvecs, const double* eel,
                      const double* mw, double pseudoC, uint64_t seed, double confidence, int32_t m,
                      const int32_t* gene_starts, int32_t m_trans, const int32_t* trans_starts, float* tpm_ci,
                      float* fpkm_ci, float* gene_tpm_ci, float* gene_fpkm_ci, float* iso_tpm_ci, float* iso_fpkm_ci,
                      rsem_ci_profile* prof);
/* The same with the samples GIVEN: tpm_samples M x nSamples float (row j-1 = transcript j, TPM), l_bars nSamples -- the layout of
 * the reference's temporary file (Buffer.h:66-80).  For a caller that draws them itself: rsem-calculate-credibility-intervals
 * --ci-stream reference reproduces the reference's per-thread MT19937 + boost gamma draws on the host (csrc/host/ci_stream.hpp:
 * a stream whose consumption depends on the values drawn cannot be cut into device-sized pieces) and hands them over here. */
int rsem_ci_calculate_samples(int device, int32_t M, int32_t nSamples, const float* tpm_samples, const float* l_bars, double confidence,
                              int32_t m, const int32_t* gene_starts, int32_t m_trans, const int32_t* trans_starts, float* tpm_ci,
                              float* fpkm_ci, float* gene_tpm_ci, float* gene_fpkm_ci, float* iso_tpm_ci, float* iso_fpkm_ci,
                              rsem_ci_profile* prof);
/* The sampling stage alone (tests): tpm_samples M x (nCV*nSpC) float, row j-1 = transcript j, as the reference's
 * temporary file (Buffer.h:66-80); l_bars nCV*nSpC. */
int rsem_ci_sample(int device, int32_t M, int32_t nCV, int32_t nSpC, const int32_t* cvecs, const double* eel,
                   const double* mw, double pseudoC, uint64_t seed, float* tpm_samples, float* l_bars);
/* The interval stage alone: nrows rows of nSamples floats (host, not modified) -> lb, ub, cqv [nrows]
 * (calcCI, calcCI.cpp:216-284). */
int rsem_ci_intervals(int device, int64_t nrows, int32_t nSamples, const float* rows, double confidence, float* lb,
                      float* ub, float* cqv);
/* The interval stage of the three calls above takes its rows in batches of at most 2^30 keys.  The environment variable
 * RSEM_CI_BATCH_KEYS (a whole number from nSamples to 2^30; anything else: RSEM_ERR_INVALID), read at every call, replaces
 * the 2^30 (a test knob: the results do not depend on it). */

/* ---- shared k-mers (rsem-for-ebseq-calculate-clustering-info) ----------------------------------------------
 * Replaces the sort-and-count of EBSeq/calcClusteringInfo.cpp:101-130.  codes: the transcripts' bases one after the other, one
 * byte per base, 0 .. 4 = A C G T N (N is an ordinary fifth letter); transcript t is codes[seq_off[t] .. seq_off[t+1]).
 * shared[t]: the number of k-mer start positions of transcript t whose k-mer also occurs in at least one OTHER transcript (a
 * k-mer repeated only inside one transcript counts nothing; one that is repeated inside and occurs elsewhere counts every one of
 * its positions).  Integer arithmetic: the result does not depend on any order.  Needs no context.
 * Checked before the device is touched (RSEM_ERR_INVALID): k >= 1, seq_off[0] = 0 and never decreasing, no transcript of 2^32
 * bases, every code <= 4.  Where no transcript is as long as k the answer is all zeros and the device is not touched either;
 * otherwise k above 32768 is refused (RSEM_ERR_INVALID).
 * Keys, sort values and their double buffers take 24 bytes per k-mer (32 once the bases and one separator per transcript pass
 * 2^32): the library sorts back and forth between the two halves, and its own temporary storage, asked of it for the size in
 * question, is counted on top.  Where that exceeds the free device memory less a margin, the k-mers are cut into batches by the value of their first
 * min(k, 8) bases: whole buckets in ascending order while they stay within the budget, a bucket above the budget a batch of its
 * own; a batch that does not fit the device, or holds 2^31 k-mers, fails with RSEM_ERR_NOMEM before anything is sorted.  The
 * environment variable RSEM_KMER_BATCH_ITEMS (a whole number >= 1; anything else: RSEM_ERR_INVALID), read at every call, replaces
 * the budget (a test knob: the results do not depend on it, n_batches does).  RSEM_KMER_WIDE_VALUES = 1 (0 or 1; anything else:
 * RSEM_ERR_INVALID) sorts by 64-bit positions whatever the length (a test knob: small inputs through the path of 2^32 bases). */
typedef struct rsem_kmer_info {
    uint64_t n_kmers, n_groups;   /* k-mer start positions; distinct k-mers */
    int32_t n_batches, n_chunks;  /* n_chunks = ceil(k / 27): sorts per batch */
    uint64_t batch_items;         /* the budget in force */
    uint64_t max_batch_items;     /* the largest batch */
    uint64_t batch_bytes;         /* device bytes of the batch buffers: the halves of keys and values and the library's temporary storage */
    double upload_ms;             /* bases and offsets to the device */
    double kernel_ms;             /* from there to the last counter: kernels, library sorts and scans, the batches' hand-offs */
} rsem_kmer_info;
int rsem_kmer_shared_counts(int device, int32_t M, const uint64_t* seq_off /* M+1 */, const uint8_t* codes, int32_t k,
                            uint32_t* shared /* M */, rsem_kmer_info* info /* may be NULL */);

/* ---- per-base read depth (rsem-bam2wig, rsem-bam2readdepth) -------------------------------------------------
 * Replaces the loop of wiggle.cpp:16-37 (`read_depth[pos] += w` once per aligned base, on one thread).  Block i covers the bases
 * start[i] .. start[i] + len[i] - 1 with the weight w[i]; the blocks are given in record order.  depth[b] becomes the FOLD
 * ((depth[b] + w[i1]) + w[i2]) + ..., over the blocks i1 < i2 < ... that cover base b, in that order, continued from the value
 * passed in -- bit for bit what the reference's loop leaves, whose sums depend on the order of their additions.  No floating-point
 * atomic, prefix sum or tree takes part.  Needs no context.
 * Checked before the device is touched (RSEM_ERR_INVALID): start[i] + len[i] <= n_bases for every block, without overflow.
 * n_blocks == 0 or n_bases == 0 leaves depth as it is and does not touch the device; neither do blocks that all have len 0.
 * The bases are cut into tiles of 512; a block makes one entry per tile it touches; a stable radix sort on the tile groups the entries
 * and keeps the blocks' order inside a tile; one workgroup per touched tile folds.  The blocks go through in batches, in their order:
 * whole blocks while their items (a block's entries, 1 for a block without bases) stay within the budget of 2^26, a block above the
 * budget a batch of its own.  depth stays on the device from the first batch to the last: n_bases doubles, 28 bytes per block and
 * 28 per entry of the largest batch and the library's temporary storage have to fit (RSEM_ERR_NOMEM before anything is allocated);
 * a caller with more bases than that calls once per stretch of them.  The environment variable RSEM_DEPTH_BATCH_ITEMS (a whole
 * number >= 1; anything else: RSEM_ERR_INVALID), read at every call, replaces the budget (a test knob: the results do not depend
 * on it, n_batches does). */
typedef struct rsem_depth_info {
    uint64_t n_entries;        /* (block, tile) pairs */
    uint64_t n_tiles_touched;  /* summed over the batches: a tile that two batches touch counts twice */
    int32_t n_batches;
    int32_t n_launches;        /* kernels and library calls: seven per batch that has entries, whatever the blocks are */
    uint64_t batch_items;      /* the budget in force */
    uint64_t device_bytes;     /* allocated for the call */
    double upload_ms;          /* depth and the batches' blocks to the device */
    double kernel_ms;          /* the batches' kernels, sorts and scans */
} rsem_depth_info;
int rsem_depth_accumulate(int device, uint64_t n_bases, uint64_t n_blocks, const uint64_t* start, const uint32_t* len, const double* w,
                          double* depth /* n_bases, in and out */, rsem_depth_info* info /* may be NULL */);

/* ---- transcript coordinates -> genome coordinates, and the per-read collapse (rsem-tbam2gbam) -----------------
 * rsem_gmap_create keeps the reference of BamConverter (BamConverter.h:45-73, Transcripts of a type-0 .ti): per transcript its
 * strand ('+' or '-'), its length without poly-A tail, the tid of its chromosome in the output header, and its exons
 * exon_off[t] .. exon_off[t + 1] - 1 of the flat arrays (1-based, inclusive, ascending).  Refused (RSEM_ERR_INVALID): a negative
 * count or tid, another strand, a transcript without exons or with more than 32766 (n_cigar is 16 bits in BAM), exons that are
 * empty, overlap or descend, exons whose bases do not add up to `length` (tr2chr walks the exons AND uses the length: sam_utils.h:
 * 138-181).  Nothing is uploaded before the first rsem_gmap_convert that has an alignment: creating needs no device.
 *
 * rsem_gmap_convert takes whole groups -- group g is the alignments group_off[g] .. group_off[g + 1] - 1, the consecutive records of
 * one read -- of single-end (mates = 1) or paired-end (mates = 2) alignments; the mates of alignment a are a * mates and
 * a * mates + 1 of the per-mate arrays, read 1 first.  No names, sequences or tags are passed.
 *   per mate, replacing convert + tr2chr (BamConverter.h:150-191, sam_utils.h:137-208) and bam_endpos / hts_reg2bin of htslib 1.3
 *   (sam.c:327-342): the range pos + 1 .. pos + l_qseq of transcript tr (the record's own CIGAR is ignored), mirrored on a '-'
 *   transcript, becomes out_tid, out_pos (0-based), out_n_cigar alternating M / N words with I for the bases off either end of the
 *   transcript (one I for a read wholly in the poly-A tail), out_bin, out_has_n (the CIGAR has an N: XS:A is due); out_flag is flag
 *   with 0x10 flipped on '-', and 0x20 too where 0x1 is set.  The words of mate i are cigar_words[cigar_off[i] .. cigar_off[i + 1]);
 *   cigar_off has one element more than there are mates.  cigar_cap is the room in cigar_words: the sum over the mates of
 *   2 * (exons of the transcript) + 2 always suffices; less than what is needed is RSEM_ERR_INVALID.
 *   per group, replacing CollapseMap (bc_aux.h:9-118) and the order of writeCollapsedLines (BamConverter.h:193-218): alignments
 *   whose converted (tid, pos, reverse bit, n_cigar, CIGAR words) of mate 1, then of mate 2, are equal become one, the first in
 *   file order; its weight is the float fold w_first + w_next + ... in file order; the group comes out in the order of that key.
 *   out_src[k] is the alignment (index in the call) that is written k-th and out_w[k] its folded weight; both have room for
 *   n_alignments, info->n_alignments_out say how many count; the groups come out in their order.
 * MAPQ is not computed here: it is glibc's log10 of the folded float on the host (sam_utils.h:72-76).
 * Checked before a device is touched (RSEM_ERR_INVALID): a NULL handle, mates other than 1 or 2, negative counts, group_off that
 * does not start at 0, end at n_alignments and strictly ascend, a transcript index outside the reference, pos < 0, l_qseq < 1.
 * The groups go through in batches: whole groups in order while their alignments stay within the budget of 2^22, a group above the
 * budget a batch of its own.  The environment variable RSEM_GMAP_BATCH_ITEMS (a whole number >= 1; anything else:
 * RSEM_ERR_INVALID), read at every call, replaces the budget (a test knob: the results do not depend on it, n_batches does).
 * The handle's device buffers grow to the largest batch seen and are kept; calls on one handle are serialised. */
typedef struct rsem_gmap rsem_gmap;
typedef struct rsem_gmap_info {
    uint64_t n_groups;
    uint64_t n_alignments_in;
    uint64_t n_alignments_out;
    uint64_t n_cigar_words;
    int32_t n_batches;
    int32_t n_launches;        /* kernels and library scans: six per batch */
    uint64_t batch_items;      /* the budget in force */
    uint64_t device_bytes;     /* held by the handle after the call */
    double upload_ms;          /* the batches' fields to the device */
    double kernel_ms;          /* the batches' kernels and scans */
} rsem_gmap_info;
int rsem_gmap_create(rsem_gmap** out, int device, int32_t n_transcripts, const uint8_t* strand, const int32_t* length, const int32_t* out_tid,
                     const uint64_t* exon_off /* n_transcripts + 1 */, const int32_t* exon_start, const int32_t* exon_end);
int rsem_gmap_convert(rsem_gmap* h, int32_t mates, int64_t n_alignments, int64_t n_groups, const uint64_t* group_off /* n_groups + 1 */,
                      const int32_t* tr, const int32_t* pos, const int32_t* l_qseq, const uint32_t* flag /* per mate */,
                      const float* w /* per alignment */, int32_t* out_tid, int32_t* out_pos, uint32_t* out_flag, uint32_t* out_n_cigar,
                      uint32_t* out_bin, uint32_t* out_has_n /* per mate */, uint64_t* cigar_off /* mates + 1 */, uint32_t* cigar_words,
                      uint64_t cigar_cap, uint64_t* out_src, float* out_w /* n_alignments */, rsem_gmap_info* info /* may be NULL */);
void rsem_gmap_destroy(rsem_gmap* h);

/* ---- FASTA bodies -> bases, segments of bases -> sequences (rsem-extract-reference-transcripts, rsem-synthesis-reference-transcripts,
 * rsem-preref) ----------------------------------------------------------------------------------------------------------------
 * A handle owns an output store of store_bytes bytes on the device, the batch of records that is resident, and its buffers.
 * rsem_refseq_create touches no device memory.  The environment variable RSEM_REFSEQ_STORE_PAD (a whole number of bytes, a
 * multiple of 16; anything else: RSEM_ERR_INVALID), read there, puts that many device bytes in front of the store: they are
 * allocated, never written and never read, and count into every address (a few hundred bases on both sides of 2^32).
 *
 * rsem_refseq_load replaces the getline / check / += loops over a record's body (extractRef.cpp:336-349, synthesisRef.cpp:175-188:
 * mode 1, checked; Refs.h:96-102: mode 0, raw).  The host has found the header lines: record r's body is raw[body_lo[r], body_hi[r]),
 * the bodies ascend and lie apart, what lies between them is not looked at.  Records first, first + 1, ... are taken while the raw
 * bytes from the first body's start to the last one's end stay within the budget -- a quarter of the free device memory, or the
 * environment variable RSEM_REFSEQ_BATCH_BYTES (a whole number from 1 on; anything else: RSEM_ERR_INVALID), read at every call; a
 * record above the budget is a batch of its own -- and *n_taken says how many.  For each of them the device drops the '\n' bytes and
 * leaves the bases contiguous; n_bases[r] is their number (0 for a record with keep[r] == 0, which is checked but not kept; keep
 * may be NULL: all are kept).  In checked mode a letter other than A, C, G, T, a, c, g, t becomes N or n by its case (check,
 * extractRef.cpp:297-303) and bad[r] is the offset into raw of the body's first byte that is no letter, or -1; in raw mode the bytes
 * stay and bad[r] is -1.  The batch stays resident until the next load.  Refused before anything is uploaded: a record of more than
 * 2^31 - 1 bases (the reference's coordinates are int).
 *
 * rsem_refseq_gather replaces Transcript::extractSeq (Transcript.h:90-117), RefSeqPolicy::convert (RefSeqPolicy.h:11-19),
 * AlignerRefSeqPolicy::convert and the poly-A append of RefSeq.h:23-28: segment i is len[i] bases of the resident record src[i] (its
 * index in the load call's arrays) from base first_base[i] (0-based) on, written to the store at dst[i].  flags: 1 the segment is
 * read backwards through getOpp (utils.h:78-94); 2 upper case, and N for anything but A, C, G, T; 4 N becomes G after that; 8 the
 * segment is len[i] times 'A' (src and first_base are not looked at).  The destinations must ascend and lie apart (every output byte
 * has one writer); a segment outside its record or the store is RSEM_ERR_INVALID, before any launch.
 * rsem_refseq_download copies bytes of the store to the host.  Calls on one handle are serialised. */
typedef struct rsem_refseq rsem_refseq;
typedef struct rsem_refseq_info {  /* sums over the handle's calls */
    uint64_t n_records;
    uint64_t raw_bytes;        /* uploaded and read twice by the load kernels */
    uint64_t n_bases;          /* written by the load, kept records only */
    uint64_t n_segments;
    uint64_t gathered_bytes;   /* written by the gather (and read, but for the fills) */
    int32_t n_batches;         /* loads */
    int32_t n_launches;        /* kernels and library scans: three a load, one a gather */
    uint64_t batch_bytes;      /* the budget of the last load */
    uint64_t store_pad;
    uint64_t device_bytes;     /* held by the handle */
    double upload_ms;
    double kernel_ms;
    double download_ms;
} rsem_refseq_info;
#define RSEM_REFSEQ_RAW 0
#define RSEM_REFSEQ_CHECKED 1
#define RSEM_REFSEQ_RC 1u
#define RSEM_REFSEQ_UPPER_N 2u
#define RSEM_REFSEQ_N2G 4u
#define RSEM_REFSEQ_FILL 8u
int rsem_refseq_create(rsem_refseq** out, int device, uint64_t store_bytes);
int rsem_refseq_load(rsem_refseq* h, int32_t mode, const uint8_t* raw, int64_t n_records, const uint64_t* body_lo, const uint64_t* body_hi,
                     const uint8_t* keep /* may be NULL */, int64_t first, int64_t* n_taken, uint64_t* n_bases /* n_records */, int64_t* bad /* n_records */);
int rsem_refseq_gather(rsem_refseq* h, int64_t n_segments, const int64_t* src, const uint32_t* first_base, const uint32_t* len, const uint64_t* dst,
                       const uint32_t* flags);
int rsem_refseq_download(rsem_refseq* h, uint64_t offset, uint64_t bytes, uint8_t* out);
int rsem_refseq_get_info(rsem_refseq* h, rsem_refseq_info* info);
void rsem_refseq_destroy(rsem_refseq* h);

/* ---- the checks of a name-grouped alignment file (rsem-sam-validator, rsem-get-unique) -----------------------------------------
 * rsem_alncheck_create keeps target_len (bam_hdr_t::target_len, samValidator.cpp:45,143) and touches no device.
 *
 * rsem_alncheck_push is a stream: the records of one push continue those of the pushes before.  It replaces the loop of
 * samValidator.cpp:82-183 with check_read (:26-59).  Record i has the name names[name_off[i] .. name_off[i + 1]) (no NUL), its BAM
 * fields flag, tid, pos, isize, l_qseq, and the CIGAR words cigar[cigar_off[i] .. cigar_off[i + 1]).  The first record of the first push
 * fixes the mode (:91): flag & 1 set means paired.  A unit is one record, or in paired mode the records 2k and 2k + 1 of the file (:101);
 * a push in paired mode holds an even number of records unless `last` is set.  Per unit, the first check that fails, in the
 * reference's order (:93-164): MIXED, ONE_MATE (no second record, other canonical name, second not flagged paired), SAME_MATE_NUMBER,
 * ONE_MATE_ALIGNED, then with both mates aligned and read 1 first DISCORDANT, SAME_STRAND, PAIR_BOUNDARY (the mate of smaller pos:
 * pos >= 0 && pos + |isize| <= target_len, in 64 bits), check_read of read 1, check_read of read 2; single-end, if mapped, check_read.
 * check_read (:26-59): the first offending CIGAR operation in CIGAR order -- CIGAR_SKIP for N, CIGAR_INDEL for I or D, CIGAR_CLIP for
 * S, H or P -- then BOUNDARY: pos < 0 or bam_endpos of htslib 1.3 (sam.c:336-342: pos + the reference-consuming lengths, pos + 1 for a
 * record without CIGAR) above target_len[tid].  After the unit's own checks those of its group (:166-178); a unit's name is its first
 * record's canonical name, the bytes before the first of " \t\n\r\f\v" (sam_utils.h:45,54-61; cut on the device): a unit whose name
 * differs from the unit before opens a group, NOT_GROUPED if an earlier group of the file has exactly that name (the std::set `used`,
 * :22,167-169); a unit that continues a group repeats the l_qseq of the unit before (read 1's and read 2's in paired mode), else
 * DIFFERENT_LENGTHS (:176).  The verdict is the failing unit of smallest index: where the reference stops.  Once a verdict with
 * code != 0 has been returned, or after a push with `last`, further pushes are refused (RSEM_ERR_STATE).
 * NOT_GROUPED is exact: every group's name stays on the device (its bytes and 16 bytes a group: a 64-bit hash and where the name
 * lies), a batch's groups as a run sorted by (hash, group); equal hashes are settled by comparing the bytes.  When they no longer fit:
 * RSEM_ERR_NOMEM, with what is resident kept.
 * Checked before a device is touched (RSEM_ERR_INVALID): a NULL handle or verdict, negative counts, name_off / cigar_off that do not
 * start at 0 and ascend, a name of 0 or more than 254 bytes or one that starts with white space (the reference's assert at :175),
 * more than 65535 CIGAR operations, l_qseq < 1 (its assert at :86,107), a mapped record whose tid is outside the targets (:45 reads
 * outside its arrays there), an odd number of paired-end records without `last`.
 * The environment variables RSEM_ALNCHECK_BATCH_ITEMS (a whole number >= 1) and RSEM_ALNCHECK_HASH_BITS (1 .. 64: only that many bits
 * of the hash are kept -- collisions on purpose), read at every call (anything else: RSEM_ERR_INVALID), replace the batch budget of
 * 2^22 records and the hash width: test knobs, the verdicts do not depend on them.
 *
 * rsem_alncheck_unique is stateless and takes whole groups; it replaces output() of getUnique.cpp:25-30 and the grouping of :55-65:
 * groups are runs of equal RAW names; keep[i] = 1 iff no record of i's group has flag & 4 and the group has 2 records where its first
 * has flag & 1, else 1.  It takes the batch knob (the end of a batch moves behind the group it would cut). */
#define RSEM_ALNCHECK_OK 0
#define RSEM_ALNCHECK_MIXED 1
#define RSEM_ALNCHECK_ONE_MATE 2
#define RSEM_ALNCHECK_SAME_MATE_NUMBER 3
#define RSEM_ALNCHECK_ONE_MATE_ALIGNED 4
#define RSEM_ALNCHECK_DISCORDANT 5
#define RSEM_ALNCHECK_SAME_STRAND 6
#define RSEM_ALNCHECK_PAIR_BOUNDARY 7
#define RSEM_ALNCHECK_CIGAR_SKIP 8
#define RSEM_ALNCHECK_CIGAR_INDEL 9
#define RSEM_ALNCHECK_CIGAR_CLIP 10
#define RSEM_ALNCHECK_BOUNDARY 11
#define RSEM_ALNCHECK_NOT_GROUPED 12
#define RSEM_ALNCHECK_DIFFERENT_LENGTHS 13
typedef struct rsem_alncheck rsem_alncheck;
typedef struct rsem_alncheck_verdict {
    int32_t code;              /* 0 = nothing wrong so far, else RSEM_ALNCHECK_* */
    int32_t mate;              /* which record of the unit the message names (0 / 1) */
    int64_t unit_record;       /* index in this push of the failing unit's first record; -1 if code == 0 */
    uint64_t units_ok;         /* units counted before the stop (the reference's cnt): this push only */
    uint32_t cigar_op;         /* the offending operation's letter for the CIGAR codes */
    int32_t paired;            /* the mode: 0 / 1, -1 before the first record */
    uint64_t n_records;        /* of this push */
    uint64_t n_units;
    uint64_t n_groups;         /* opened by this push */
    uint64_t resident_groups;  /* of the handle */
    uint64_t resident_name_bytes;
    int32_t n_batches;
    int32_t n_launches;        /* kernels and library calls: three a batch, five where it opens a group */
    uint64_t batch_items;      /* the budget in force */
    uint64_t device_bytes;     /* held by the handle after the call */
    double upload_ms;
    double kernel_ms;          /* the batches' kernels, scans and sorts */
} rsem_alncheck_verdict;
typedef struct rsem_alncheck_info {
    uint64_t n_records;
    uint64_t n_groups;
    uint64_t n_kept;
    int32_t n_batches;
    int32_t n_launches;        /* three a batch */
    uint64_t batch_items;
    uint64_t device_bytes;     /* held during the call */
    double upload_ms;
    double kernel_ms;
} rsem_alncheck_info;
int rsem_alncheck_create(rsem_alncheck** out, int device, int32_t n_targets, const uint32_t* target_len);
int rsem_alncheck_push(rsem_alncheck* h, int64_t n_records, const uint64_t* name_off /* n + 1 */, const uint8_t* names, const uint32_t* flag,
                       const int32_t* tid, const int32_t* pos, const int32_t* isize, const int32_t* l_qseq, const uint64_t* cigar_off /* n + 1 */,
                       const uint32_t* cigar, int32_t last, rsem_alncheck_verdict* v);
void rsem_alncheck_destroy(rsem_alncheck* h);
int rsem_alncheck_unique(int device, int64_t n_records, const uint64_t* name_off /* n + 1 */, const uint8_t* names, const uint32_t* flag,
                         uint8_t* keep /* n_records */, rsem_alncheck_info* info /* may be NULL */);

/* ---- mates made adjacent (rsem-scan-for-paired-end-reads) --------------------------------------------------------------------------
 * rsem_pairscan_create touches no device.  rsem_pairscan_reorder replaces the loop of scanForPairedEndReads.cpp:78-126 with
 * add_to_appropriate_arr (:24-32), get_pattern_code (:34-37) and less_than (:39-51) for records that are grouped by read name: record i
 * has the name names[name_off[i] .. name_off[i + 1]) (no NUL) and its BAM fields flag, tid, pos, mpos.  A call takes whole runs of
 * equal canonical names (the bytes before the first of " \t\n\r\f\v", sam_utils.h:45,54-61): no group crosses such a boundary.
 * perm_out[k] is the index in this call of the k-th record the reference writes.
 * Groups (:79-87, :117-122): a group opens at a record s, its name is the canonical name of s, its mode bit 0x1 of s's flag.  A
 * single-end group runs on while the next record's RAW name equals that name and is written as it comes; a paired group runs on while
 * the next record's CANONICAL name equals it.  On the device a record opens a group iff its canonical name differs from the record
 * before (a hard start), or its raw name is longer than its canonical name and none of the hard start and the such records before it
 * in its run has bit 0x1 -- a prefix count.
 * A paired group (:83-115): its records are `both` (!(flag & 4) && (flag & 2)), partial_1 (else flag & 0x40), partial_2 (else flag &
 * 0x80) or unknown.  First the `both` records sorted by less_than -- tid, min(pos, mpos), max(pos, mpos), then the pattern code (read 1: 0
 * forward, 1 reverse; any other record: 1 forward, 0 reverse), all signed 32-bit -- STABLY: records that tie keep their order (the
 * reference's std::sort leaves the order inside a tie to the library; up to 16 records it is an insertion sort and gives this
 * order).  Then, each vector from its back: partial_1 and partial_2 in turns while both last, then what is left of one of them, each
 * with the last unknown behind it, then the other unknown records.
 * The verdict is the failing group of smallest index in the call, with the reference's first complaint about it: MIXED (a record
 * without bit 0x1 in a paired group, :85), ODD_FULL (:89), ODD_PARTIAL (:90), and NO_PARTNER where the reference calls back() on an
 * empty vector (:105,109: more left-over partial records than unknown ones).  With code != 0 perm_out is unspecified, and nothing
 * runs behind the failing batch.
 * The handle keeps its stream and its buffers between calls and grows them to the largest batch.  After a call with `last` it takes
 * no more records (RSEM_ERR_STATE).
 * Checked before a device is touched (RSEM_ERR_INVALID): a NULL handle, perm_out or verdict, negative counts, 2^32 records or more,
 * name_off that does not start at 0 and ascend, a name of 0 or more than 254 bytes.
 * The environment variable RSEM_PAIRSCAN_BATCH_ITEMS (a whole number >= 1, read at every call, anything else: RSEM_ERR_INVALID)
 * replaces the batch budget of 2^22 records; a batch is whole runs of equal canonical names within the budget, a run above it is a
 * batch of its own.  The results do not depend on it, n_batches does. */
#define RSEM_PAIRSCAN_OK 0
#define RSEM_PAIRSCAN_MIXED 1
#define RSEM_PAIRSCAN_ODD_FULL 2
#define RSEM_PAIRSCAN_ODD_PARTIAL 3
#define RSEM_PAIRSCAN_NO_PARTNER 4
typedef struct rsem_pairscan rsem_pairscan;
typedef struct rsem_pairscan_verdict {
    int32_t code;              /* 0 = nothing wrong, else RSEM_PAIRSCAN_* */
    int32_t n_batches;
    int64_t group;             /* the failing group's index among this call's groups; -1 if code == 0 */
    int64_t group_record;      /* index in this call of its first record; -1 if code == 0 */
    uint64_t n_records;        /* of this call */
    uint64_t n_groups;         /* of this call; with code != 0: of the batches that ran */
    uint64_t n_sorted_groups;  /* groups with two or more `both` records */
    int32_t n_launches;        /* kernels and library calls: ten a batch, eleven where a group is sorted */
    int32_t reserved;
    uint64_t batch_items;      /* the budget in force */
    uint64_t device_bytes;     /* held by the handle after the call */
    double upload_ms;
    double kernel_ms;          /* the batches' kernels and scans */
} rsem_pairscan_verdict;
int rsem_pairscan_create(rsem_pairscan** out, int device);
int rsem_pairscan_reorder(rsem_pairscan* h, int64_t n_records, const uint64_t* name_off /* n + 1 */, const uint8_t* names, const uint32_t* flag,
                          const int32_t* tid, const int32_t* pos, const int32_t* mpos, int32_t last, uint32_t* perm_out /* n_records */,
                          rsem_pairscan_verdict* v);
void rsem_pairscan_destroy(rsem_pairscan* h);

/* ---- reads drawn from the read model (rsem-simulate-reads) ---------------------------------------------------------------------------
 * A handle holds one model after startSimulation (SingleModel.h:399-411, SingleQModel.h:413-426, PairedEndModel.h:358-370,
 * PairedEndQModel.h:371-384) on one device: every table a RUNNING SUM as the reference builds it -- theta (theta_cdf), the length
 * distributions (LenDist.h: cdf[0 .. span], cdf[0] = 0), QualDist.h:116-130 (qc_init, qc_trans), the profile with its all-zero rows
 * repaired (QProfile.h:151-193, Profile.h:163-205), the noise profile (NoiseQProfile.h:153-166, NoiseProfile.h:137-144) -- the
 * RSPD's pdf and cdf of B + 2 entries (RSPD.h:182-193 is evaluated in place, not tabulated), and the transcripts' forward strands,
 * poly(A) tails included, with their two lengths.  Index 0 of the per-transcript arrays is unused.
 * A batch replaces the loop of simulation.cpp:121-126: per read, model.simulate repeated until it gives a read.  An attempt is a fixed
 * program of uniforms (rsem_amd/csrc/simulate_block.hpp); uniform k of an attempt is 32-bit word k of its source times 2^-32.
 *   rsem_sim_counter_batch     word k of attempt a of read r: word k % 4 of Philox4x32-10 keyed (seed low, seed high) at counter (r low,
 *                              r high, a, k / 4).  Reads first_read .. first_read + n_reads - 1: a pure function of seed and read.
 *   rsem_sim_reference_begin   seeds boost::random::mt19937 as simul.h:11 does;
 *   rsem_sim_reference_batch   the next up to max_reads reads of that ONE stream, in stream order: the reads, and through them every file
 *                              of the program, are the reference's for the same seed.  The stream is searched in chunks: an attempt is tried
 *                              at EVERY word of a chunk, then the words the stream really visits are found (tiles, a hop, a prefix sum).
 * Both fill the caller's arrays for reads 0 .. n_reads - 1 of the batch: sid, dir, pos, insert_l, len1, len2, the failed attempts
 * before the read (attempts), and the letters and qualities (value + 33) of read i at byte i * stride of seq1, qual1, seq2, qual2.  A
 * model without qualities leaves qual1 / qual2 alone, a single-end one seq2 / qual2 and len2 (0).  The handle adds the reads to its
 * per-transcript counts (simulation.cpp:124) and the failed attempts to its total (:122).
 * status: RSEM_SIM_ATTEMPT_CAP: a read failed the cap's number of attempts (2^20; the reference would go on for ever);
 * RSEM_SIM_SHORT_INSERT: a paired-end insert shorter than every mate length (PairedEndQModel.h:415-417 goes on with a length of -1);
 * RSEM_SIM_PAST_PROFILE: a read longer than the no-quality profile (Profile.h:211 reads past its table); RSEM_SIM_QUALITY_RANGE: a
 * quality above 93 was drawn (the tables have 100 rows; the reference ends at the assertion of QProfile.h:40).  With status != 0 the batch's
 * arrays are unspecified, nothing is added to the counts and the handle takes no more batches (RSEM_ERR_STATE).
 * Checked before a device is touched (RSEM_ERR_INVALID): NULL pointers, a type outside 0..3, M < 1, tables that a model of the type
 * needs and that are NULL, lengths that do not fit (lb < ub, 1 <= full_len <= tot_len, seq_off ascending by tot_len at least), running
 * sums that descend or are not finite, a batch whose capacity is below the reads asked for or whose stride is below the longest read.
 * Knobs (environment, whole numbers, read at every call, anything else: RSEM_ERR_INVALID; the reads do not depend on them):
 * RSEM_SIM_BATCH_READS (2^18) the reads the program asks for at a time, RSEM_SIM_CHUNK_WORDS (2^22) the words of a chunk,
 * RSEM_SIM_TILE (2048, at most 8192) the positions of a tile, RSEM_SIM_ATTEMPT_CAP (2^20), RSEM_SIM_LDS_TABLES (1) the quality tables
 * in LDS (1) or read through the caches (0). */
#define RSEM_SIM_OK 0
#define RSEM_SIM_ATTEMPT_CAP 1
#define RSEM_SIM_SHORT_INSERT 2
#define RSEM_SIM_PAST_PROFILE 3
#define RSEM_SIM_QUALITY_RANGE 4
typedef struct rsem_sim rsem_sim;
typedef struct rsem_sim_model {
    int32_t type;               /* 0 Single, 1 SingleQ, 2 PairedEnd, 3 PairedEndQ */
    int32_t M;
    int32_t has_mld;            /* single-end: m_cdf is given; paired-end: must be 1 */
    int32_t est_rspd, B;
    int32_t pro_len;            /* no-quality models: positions of pc */
    int32_t g_lb, g_ub, m_lb, m_ub;
    double prob_f;              /* Orientation.h:36 */
    const double* theta_cdf;    /* M + 1 */
    const int32_t* full_len;    /* M + 1 */
    const int32_t* tot_len;     /* M + 1 */
    const uint64_t* seq_off;    /* M + 2 */
    const uint8_t* seq;         /* seq_off[M + 1] bytes */
    const double* g_cdf;        /* g_ub - g_lb + 1 */
    const double* m_cdf;        /* m_ub - m_lb + 1, or NULL */
    const double* r_pdf;        /* B + 2 (est_rspd only) */
    const double* r_cdf;
    const double* qc_init;      /* 100 (quality models only) */
    const double* qc_trans;     /* 100 * 100 */
    const double* pc;           /* 100 * 25, or pro_len * 25 */
    const double* npc;          /* 100 * 5, or 5 */
} rsem_sim_model;
typedef struct rsem_sim_batch {
    int64_t capacity;           /* in: reads the arrays hold */
    int32_t stride;             /* in: bytes a read in seq1, qual1, seq2, qual2 */
    int32_t status;             /* RSEM_SIM_* */
    int64_t n_reads;            /* reads in the arrays */
    uint64_t resimulations;     /* failed attempts of this batch */
    int32_t *sid, *dir, *pos, *insert_l, *len1, *len2;
    uint32_t* attempts;
    uint8_t *seq1, *qual1, *seq2, *qual2;
    int32_t n_chunks;           /* reference stream: chunks searched */
    int32_t n_launches;
    uint64_t stream_words;      /* reference stream: generator words the batch consumed */
    uint64_t device_bytes;
    double words_ms;            /* host: the generator */
    double upload_ms;           /* device, by events: the words going up */
    double search_ms;           /* device: an attempt's header at every word, tiles, hop, marks, prefix sum */
    double body_ms;             /* device: the reads */
    double download_ms;         /* host clock: the arrays coming back */
} rsem_sim_batch;
typedef struct rsem_sim_knobs {
    uint64_t batch_reads, chunk_words, tile, attempt_cap, lds_tables;
} rsem_sim_knobs;
int rsem_sim_read_knobs(rsem_sim_knobs* k);
/* the longest read of the model and whether every sample() of it takes one uniform (what the search of the reference stream can skip) */
int rsem_sim_create(rsem_sim** out, const rsem_sim_model* m, int device);
int rsem_sim_info(const rsem_sim* h, int32_t* max_len, int32_t* plain);
int rsem_sim_counter_batch(rsem_sim* h, uint64_t seed, uint64_t first_read, int64_t n_reads, rsem_sim_batch* b);
int rsem_sim_reference_begin(rsem_sim* h, uint32_t seed);
int rsem_sim_reference_batch(rsem_sim* h, int64_t max_reads, rsem_sim_batch* b);
/* counts: M + 1 (simulation.cpp:124); resimulations: the total of :122 */
int rsem_sim_totals(rsem_sim* h, uint64_t* counts, uint64_t* resimulations);
void rsem_sim_destroy(rsem_sim* h);

#ifdef __cplusplus
}
#endif
#endif /* RSEM_HIP_H_ */
