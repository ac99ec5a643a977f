// pairscan_host.hpp -- the host side of rsem-scan-for-paired-end-reads (scanForPairedEndReads.cpp): records -> fields, the device
// call (rsem_pairscan_reorder, rsem_amd/csrc/pairscan.hip), the messages, BGZF out.  DESIGN.md section 15.
//
// The reference reads, groups, sorts and writes record by record on one thread (its threads only deflate).  Here
//   read      SAM text or BAM in super-chunks (AlignmentReader, RecordChunks: BGZF blocks inflated side by side);
//   hold      the trailing run of equal canonical names waits for the next super-chunk: a group never crosses such a boundary;
//   fields    per record name, flag, tid, pos, mpos -- on the threads;
//   device    the order the reference writes the records in, and the first group it would stop at;
//   output    the records as they are, gathered in that order and deflated piece by piece on the threads.
#pragma once
#include "alncheck_host.hpp"

namespace rsemh {

// the fields of the records [0, n) for rsem_pairscan_reorder, extracted on the pool's threads
struct PairscanFields {
    std::vector<uint64_t> name_off;
    std::vector<uint8_t> names;
    std::vector<uint32_t> flag;
    std::vector<int32_t> tid, pos, mpos;

    void extract(const std::vector<RecView>& recs, StagePool& pool, const std::string& path) {
        const size_t n = recs.size();
        name_off.assign(n + 1, 0);
        flag.resize(n); tid.resize(n); pos.resize(n); mpos.resize(n);
        const size_t np = std::max<size_t>(1, std::min<size_t>((size_t)pool.threads() * 4, n / 4096 + 1));
        std::vector<uint64_t> nb(np + 1, 0);
        std::vector<int> bad(np, 0);
        pool.run(np, [&](size_t i, int) {
            uint64_t b = 0;
            for (size_t r = n * i / np, e = n * (i + 1) / np; r < e; r++) {
                if (recs[r].n < 33) { bad[i] = 1; return; }
                b += raw_name(recs[r]).second;
            }
            nb[i + 1] = b;
        });
        for (size_t i = 0; i < np; i++) {
            if (bad[i]) die("%s: an alignment record of fewer than 33 bytes", path.c_str());
            nb[i + 1] += nb[i];
        }
        names.resize((size_t)nb[np] + 1);
        pool.run(np, [&](size_t i, int) {
            uint64_t b = nb[i];
            for (size_t r = n * i / np, e = n * (i + 1) / np; r < e; r++) {
                RecCore c;
                rec_core(recs[r], c);
                const auto nm = raw_name(recs[r]);
                name_off[r] = b;
                memcpy(names.data() + b, nm.first, nm.second);
                b += nm.second;
                flag[r] = c.flag; tid[r] = c.tid; pos[r] = c.pos; mpos[r] = c.mpos;
            }
        });
        name_off[n] = nb[np];
    }
};

// what the reference says about the group it stops at (scanForPairedEndReads.cpp:85,89,90 through general_assert_1, my_assert.h:35-41:
// a line end on stdout, the message on stderr, exit(-1)); NO_PARTNER is this program's own: the reference calls back() on an empty
// vector there (:105,109)
[[noreturn]] inline void stop_at_group(int code, const RecView& first) {
    const auto nm = canonical_name(first);
    const std::string q(nm.first, nm.second);
    printf("\n");
    fflush(stdout);
    switch (code) {
        case RSEM_PAIRSCAN_MIXED: die("Read %s is detected as both single-end and paired-end read!", q.c_str());
        case RSEM_PAIRSCAN_ODD_FULL: die("Number of first and second mates in read %s's full alignments (both mates are aligned) are not matched!", q.c_str());
        case RSEM_PAIRSCAN_ODD_PARTIAL: die("Number of first and second mates in read %s's partial alignments (at most one mate is aligned) are not matched!", q.c_str());
        case RSEM_PAIRSCAN_NO_PARTNER:
            die("Read %s: its partial alignments leave a first or second mate without a record to put behind it (first mates, second mates and records that are neither "
                "do not pair up; the reference program reads an empty list here)", q.c_str());
        default: die("internal error: verdict code %d", code);
    }
}

inline void scan_for_paired_end_reads(const std::string& inF, const std::string& outF, const AlncheckOptions& opt) {
    const auto t_all = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    {
        FILE* f = fopen(inF.c_str(), "rb");
        if (!f) die("Cannot open %s !", inF.c_str());  // :61
        fclose(f);
    }
    refuse_cram(inF);
    AlignmentReader in;
    in.open(inF);
    const int nthreads = pool_threads(opt.threads);
    StagePool pool(nthreads);
    std::vector<BgzfDeflater> defl((size_t)nthreads);
    FILE* fo = fopen(outF.c_str(), "wb");
    if (!fo) die("Cannot open %s !", outF.c_str());  // :65
    uint64_t out_bytes = 0;
    {
        const std::vector<uint8_t> raw = header_bytes_as_read(inF, in);
        std::vector<uint8_t> comp;
        defl[0].stream(raw.data(), raw.size(), comp);
        if (fwrite(comp.data(), 1, comp.size(), fo) != comp.size()) die("Cannot write %s!", outF.c_str());
        out_bytes += comp.size();
    }
    printf("."); fflush(stdout);  // :76
    rsem_pairscan* ps = nullptr;
    if (const int rc = rsem_pairscan_create(&ps, opt.device)) die("%s: %s: %s", inF.c_str(), rsem_hip_strerror(rc), rsem_hip_last_error());
    size_t super_bytes = 64u << 20;
    if (const char* e = getenv("RSEM_HIP_BAM_CHUNK")) super_bytes = std::max<size_t>(64, (size_t)atoll(e));
    RecordChunks chunks(inF, in, pool, super_bytes);
    std::vector<RecView> fresh, recs;
    std::vector<std::vector<uint8_t>> held, held_next;  // the records of the run of equal canonical names that the super-chunk's end may have cut
    PairscanFields F;
    std::vector<uint32_t> perm;
    struct Piece { std::vector<uint8_t> out; };
    std::vector<Piece> pieces;
    double read_s = 0, fields_s = 0, device_s = 0, deflate_s = 0, write_s = 0, upload_ms = 0, kernel_ms = 0;
    uint64_t cnt = 0, dots = 0, records = 0, sorted = 0, calls = 0, batches = 0, launches = 0, device_bytes = 0;
    bool last = false;
    auto t0 = std::chrono::steady_clock::now();
    while (chunks.next(fresh, last)) {
        recs.clear();
        for (const auto& h : held) recs.push_back({h.data(), h.size()});
        recs.insert(recs.end(), fresh.begin(), fresh.end());
        for (const RecView& r : recs)
            if (r.n < 33) die("%s: an alignment record of fewer than 33 bytes", inF.c_str());
        size_t n = recs.size();
        if (!last && n) {  // the last run waits: a paired group goes on while the canonical names agree (:84)
            size_t k = n - 1;
            while (k > 0) {
                const auto a = canonical_name(recs[k]), b = canonical_name(recs[k - 1]);
                if (a.second != b.second || memcmp(a.first, b.first, a.second)) break;
                k--;
            }
            n = k;
        }
        held_next.clear();
        for (size_t k = n; k < recs.size(); k++) held_next.emplace_back(recs[k].d, recs[k].d + recs[k].n);
        recs.resize(n);
        read_s += since(t0);
        t0 = std::chrono::steady_clock::now();
        F.extract(recs, pool, inF);
        fields_s += since(t0);
        t0 = std::chrono::steady_clock::now();
        perm.resize(n + 1);
        rsem_pairscan_verdict v;
        const int rc = rsem_pairscan_reorder(ps, (int64_t)n, F.name_off.data(), F.names.data(), F.flag.data(), F.tid.data(), F.pos.data(), F.mpos.data(), last ? 1 : 0,
                                             perm.data(), &v);
        if (rc != RSEM_OK) die("%s: %s: %s (this program has no CPU path)", inF.c_str(), rsem_hip_strerror(rc), rsem_hip_last_error());
        device_s += since(t0);
        calls++; batches += (uint64_t)v.n_batches; launches += (uint64_t)v.n_launches; upload_ms += v.upload_ms; kernel_ms += v.kernel_ms; sorted += v.n_sorted_groups;
        device_bytes = v.device_bytes;
        if (v.code) {
            cnt += (uint64_t)v.group;  // the groups the reference has written before it stops
            for (; (dots + 1) * 1000000 <= cnt; dots++) printf(".");
            stop_at_group(v.code, recs[(size_t)v.group_record]);
        }
        t0 = std::chrono::steady_clock::now();
        const size_t np = std::max<size_t>(1, std::min<size_t>((size_t)nthreads * 4, n / 1024 + 1));
        pieces.assign(np, Piece());
        pool.run(np, [&](size_t i, int me) {
            std::vector<uint8_t> raw;
            for (size_t k = n * i / np, e = n * (i + 1) / np; k < e; k++) {
                const RecView& r = recs[perm[k]];
                const int32_t bs = (int32_t)r.n;
                raw.insert(raw.end(), (const uint8_t*)&bs, (const uint8_t*)&bs + 4);
                raw.insert(raw.end(), r.d, r.d + r.n);
            }
            defl[me].stream(raw.data(), raw.size(), pieces[i].out);
        });
        deflate_s += since(t0);
        t0 = std::chrono::steady_clock::now();
        for (Piece& P : pieces) {
            if (!P.out.empty() && fwrite(P.out.data(), 1, P.out.size(), fo) != P.out.size()) die("Cannot write %s!", outF.c_str());
            out_bytes += P.out.size();
        }
        write_s += since(t0);
        records += n;
        cnt += v.n_groups;
        for (; (dots + 1) * 1000000 <= cnt; dots++) { printf("."); fflush(stdout); }  // :125
        held.swap(held_next);
        t0 = std::chrono::steady_clock::now();
    }
    rsem_pairscan_destroy(ps);
    bgzf_write_eof(fo);
    if (fclose(fo) != 0) die("Cannot write %s!", outF.c_str());
    printf("\nFinished!\n");
    if (getenv("RSEM_HIP_TIMING"))
        printf("[timing] {\"wall_s\": %.4f, \"inflate_cut_s\": %.4f, \"fields_s\": %.4f, \"device_call_s\": %.4f, \"upload_ms\": %.3f, \"kernel_ms\": %.3f, \"gather_deflate_s\": %.4f, "
               "\"write_s\": %.4f, \"threads\": %d, \"records\": %llu, \"groups\": %llu, \"sorted_groups\": %llu, \"device_calls\": %llu, \"batches\": %llu, \"launches\": %llu, "
               "\"device_bytes\": %llu, \"out_bytes\": %llu}\n",
               since(t_all), read_s, fields_s, device_s, upload_ms, kernel_ms, deflate_s, write_s, nthreads, (unsigned long long)records, (unsigned long long)cnt,
               (unsigned long long)sorted, (unsigned long long)calls, (unsigned long long)batches, (unsigned long long)launches, (unsigned long long)device_bytes,
               (unsigned long long)out_bytes);
}

}  // namespace rsemh
