// alncheck_host.hpp -- the host side of rsem-sam-validator (samValidator.cpp) and rsem-get-unique (getUnique.cpp): records -> fields,
// the device calls (rsem_alncheck_push / rsem_alncheck_unique, rsem_amd/csrc/alncheck.hip), the messages, BGZF out.  DESIGN.md section 14.
//
// The reference reads and checks record by record on one thread.  Here
//   read      SAM text or BAM in super-chunks (AlignmentReader, RecordChunks: BGZF blocks inflated side by side);
//   fields    per record name, flag, tid, pos, isize, l_qseq and the CIGAR words -- on the -p threads;
//   device    the validator pushes every super-chunk (a record whose mate lies in the next one waits); get-unique holds back the
//             group a super-chunk's end may cut and asks which records stay;
//   output    the validator prints what the reference prints for the failing unit, whose records the super-chunk still holds;
//             get-unique writes the kept records as they are, deflated piece by piece on the -p threads.
#pragma once
#include <chrono>

#include "../../../include/rsem_hip.h"
#include "gbam_host.hpp"

namespace rsemh {

struct AlncheckOptions {
    int threads = 1, device = 0;
};

inline void refuse_cram(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) die("Cannot open %s! It may not exist.", path.c_str());
    char magic[4] = {0, 0, 0, 0};
    const size_t got = fread(magic, 1, 4, f);
    fclose(f);
    if (got == 4 && !memcmp(magic, "CRAM", 4)) die("%s is a CRAM file: CRAM input is not supported, convert it to BAM first (samtools view -b)", path.c_str());
}

inline int pool_threads(int asked) {
    int n = std::max(1, std::min(asked, (int)std::max(1u, std::thread::hardware_concurrency())));
    if (const int granted = cgroup_cpu_cores()) n = std::max(1, std::min(n, granted));
    return n;
}

// bam_get_qname as a view: the bytes before the NUL
inline std::pair<const char*, size_t> raw_name(const RecView& r) {
    const char* q = (const char*)r.d + 32;
    const size_t cap = r.n > 32 ? std::min<size_t>(r.d[8], r.n - 32) : 0;
    return {q, strnlen(q, cap)};
}

// the fields of the records [0, n) for the device calls, extracted on the pool's threads
struct RecordFields {
    std::vector<uint64_t> name_off, cigar_off;
    std::vector<uint8_t> names;
    std::vector<uint32_t> flag, cigar;
    std::vector<int32_t> tid, pos, isize, lq;

    void extract(const std::vector<RecView>& recs, StagePool& pool, bool with_cigar, const std::string& path) {
        const size_t n = recs.size();
        name_off.assign(n + 1, 0); cigar_off.assign(n + 1, 0);
        flag.resize(n); tid.resize(n); pos.resize(n); isize.resize(n); lq.resize(n);
        const size_t np = std::max<size_t>(1, std::min<size_t>((size_t)pool.threads() * 4, n / 4096 + 1));
        std::vector<uint64_t> nb(np + 1, 0), nw(np + 1, 0);
        std::vector<int> bad(np, 0);
        pool.run(np, [&](size_t i, int) {
            uint64_t b = 0, w = 0;
            for (size_t r = n * i / np, e = n * (i + 1) / np; r < e; r++) {
                RecCore c;
                if (!rec_core(recs[r], c)) { bad[i] = 1; return; }
                b += raw_name(recs[r]).second;
                if (with_cigar) w += c.n_cigar;
            }
            nb[i + 1] = b; nw[i + 1] = w;
        });
        for (size_t i = 0; i < np; i++) {
            if (bad[i]) die("%s: an alignment record is cut short", path.c_str());
            nb[i + 1] += nb[i]; nw[i + 1] += nw[i];
        }
        names.resize((size_t)nb[np] + 1);
        cigar.resize((size_t)nw[np] + 1);
        pool.run(np, [&](size_t i, int) {
            uint64_t b = nb[i], w = nw[i];
            for (size_t r = n * i / np, e = n * (i + 1) / np; r < e; r++) {
                RecCore c;
                rec_core(recs[r], c);
                const auto nm = raw_name(recs[r]);
                name_off[r] = b; cigar_off[r] = w;
                memcpy(names.data() + b, nm.first, nm.second);
                b += nm.second;
                flag[r] = c.flag; tid[r] = c.tid; pos[r] = c.pos; isize[r] = c.isize; lq[r] = c.l_seq;
                if (with_cigar) { memcpy(cigar.data() + w, recs[r].d + 32 + c.l_name, 4 * (size_t)c.n_cigar); w += c.n_cigar; }
            }
        });
        name_off[n] = nb[np];
        cigar_off[n] = nw[np];
    }
};

// ---- rsem-sam-validator ------------------------------------------------------------------------------------------------------------

// what the reference prints for the failing unit (samValidator.cpp:31-54,95-177); recs[r0] is the unit's first record
inline void print_verdict(const rsem_alncheck_verdict& v, const std::vector<RecView>& recs, const AlnHeader& H) {
    const size_t r0 = (size_t)v.unit_record;
    auto core = [&](size_t r) { RecCore c; rec_core(recs[r], c); return c; };
    auto qname = [&](size_t r) { const auto nm = raw_name(recs[r]); return std::string(nm.first, nm.second); };
    auto cname = [&](size_t r) { const auto nm = canonical_name(recs[r]); return std::string(nm.first, nm.second); };
    auto tname = [&](int32_t t) { return (t >= 0 && (size_t)t < H.names.size()) ? H.names[(size_t)t].c_str() : "*"; };
    auto tlen = [&](int32_t t) { return (t >= 0 && (size_t)t < H.lens.size()) ? H.lens[(size_t)t] : 0; };
    const size_t a = r0 + (size_t)v.mate, b = r0 + 1 - (size_t)v.mate;  // the record the message names, and the other one of a pair
    switch (v.code) {
        case RSEM_ALNCHECK_MIXED:
            printf("\nWe detected both single-end and paired-end reads in the data!\nRSEM currently does not support a mixture of single-end/paired-end reads.\n");
            break;
        case RSEM_ALNCHECK_ONE_MATE:
            printf("\nOnly find one mate for paired-end read %s!\nPlease make sure that the two mates of a paired-end read are adjacent to each other.\n", qname(r0).c_str());
            break;
        case RSEM_ALNCHECK_SAME_MATE_NUMBER:
            printf("\nThe two mates of paired-end read %s are marked as both mate1 or both mate2!\n", qname(r0).c_str());
            break;
        case RSEM_ALNCHECK_ONE_MATE_ALIGNED:
            printf("\nPaired-end read %s has an alignment with only one mate aligned!\n", qname(r0).c_str());
            printf("Currently RSEM does not handle mixed alignments for paired-end reads.\n");
            break;
        case RSEM_ALNCHECK_DISCORDANT:
            printf("\nPaired-end read %s has a discordant alignment (two mates aligned to different reference sequences)!\n", qname(a).c_str());
            printf("Mate 1 aligns to %s and mate 2 aligns to %s\n", tname(core(a).tid), tname(core(b).tid));
            printf("Currently RSEM does not handle discordant alignments.\n");
            break;
        case RSEM_ALNCHECK_SAME_STRAND:
            printf("\nPaired-end read %s has an alignment in which two mates aligned to the same strand!\n", qname(a).c_str());
            printf("Its two mates aligned to %s in %s direction.\n", tname(core(a).tid), (core(a).flag & 16) ? "reverse" : "forward");
            break;
        case RSEM_ALNCHECK_PAIR_BOUNDARY: {
            const RecCore ca = core(a), cb = core(b), t = ca.pos < cb.pos ? ca : cb;
            const int64_t span = t.isize < 0 ? -(int64_t)t.isize : (int64_t)t.isize;
            printf("\nPaired-end read %s aligns to [%d, %d) of transcript %s, which exceeds the transcript's boundary [0, %d)!\n", qname(a).c_str(), t.pos,
                   (int32_t)((int64_t)t.pos + span), tname(t.tid), tlen(t.tid));
            break;
        }
        case RSEM_ALNCHECK_CIGAR_SKIP:
            printf("\nSkipped region is detected (cigar N) for read %s!\nTo use RSEM, please align your reads to a set of transcript sequences instead of a genome.\n", qname(a).c_str());
            break;
        case RSEM_ALNCHECK_CIGAR_INDEL:
            printf("\nIndel alignment is detected (cigar %c) for read %s!\nRSEM currently does not support indel alignments.\n", (char)v.cigar_op, qname(a).c_str());
            break;
        case RSEM_ALNCHECK_CIGAR_CLIP:
            printf("\nClipping or padding is detected (cigar %c) for read %s!\nRSEM currently doest not support clipping or padding.\n", (char)v.cigar_op, qname(a).c_str());
            break;
        case RSEM_ALNCHECK_BOUNDARY: {
            const RecCore c = core(a);
            int64_t end = (int64_t)c.pos + 1;
            if (!(c.flag & 4) && c.n_cigar > 0) {
                end = c.pos;
                for (uint32_t k = 0; k < c.n_cigar; k++) {
                    uint32_t w;
                    memcpy(&w, recs[a].d + 32 + c.l_name + 4 * (size_t)k, 4);
                    if ((w & 15u) == 0 || (w & 15u) == 7 || (w & 15u) == 8) end += w >> 4;
                }
            }
            printf("\n");
            if (c.flag & 1) printf("Mate %d of paired-end read %s", (c.flag & 0x40) ? 1 : 2, qname(a).c_str());
            else printf("Read %s", qname(a).c_str());
            printf(" aligns to [%d, %d) of transcript %s, which exceeds the transcript's boundary [0, %d)!\n", c.pos, (int32_t)end, tname(c.tid), tlen(c.tid));
            break;
        }
        case RSEM_ALNCHECK_NOT_GROUPED:
            printf("\nThe alignments of read %s are not grouped together!\n", cname(r0).c_str());
            break;
        case RSEM_ALNCHECK_DIFFERENT_LENGTHS:
            printf("\nRead %s have alignments showing different read/mate lengths!\n", cname(r0).c_str());
            break;
        default: die("internal error: verdict code %d", v.code);
    }
}

inline void validate_alignments(const std::string& path, const AlncheckOptions& opt) {
    const auto t_all = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    printf("."); fflush(stdout);
    refuse_cram(path);
    AlignmentReader in;
    in.open(path);
    const AlnHeader& H = in.header;
    std::vector<uint32_t> tlen(H.lens.begin(), H.lens.end());
    rsem_alncheck* ck = nullptr;
    if (const int rc = rsem_alncheck_create(&ck, opt.device, (int32_t)tlen.size(), tlen.data())) die("%s: %s: %s", path.c_str(), rsem_hip_strerror(rc), rsem_hip_last_error());
    const int nthreads = pool_threads(opt.threads);
    StagePool pool(nthreads);
    size_t super_bytes = 64u << 20;
    if (const char* e = getenv("RSEM_HIP_BAM_CHUNK")) super_bytes = std::max<size_t>(64, (size_t)atoll(e));
    RecordChunks chunks(path, in, pool, super_bytes);
    std::vector<RecView> fresh, recs;
    std::vector<uint8_t> held;  // in paired mode: the record whose mate the next super-chunk brings
    RecordFields F;
    double read_s = 0, fields_s = 0, device_s = 0, upload_ms = 0, kernel_ms = 0;
    uint64_t cnt = 0, dots = 0, records = 0, pushes = 0, batches = 0, launches = 0, device_bytes = 0, groups = 0, name_bytes = 0;
    int paired = -1;
    bool last = false, valid = true;
    auto t0 = std::chrono::steady_clock::now();
    while (valid && chunks.next(fresh, last)) {
        recs.clear();
        if (!held.empty()) recs.push_back({held.data(), held.size()});
        recs.insert(recs.end(), fresh.begin(), fresh.end());
        if (paired < 0 && !recs.empty()) {
            if (recs[0].n < 32) die("%s: an alignment record of fewer than 32 bytes", path.c_str());
            paired = recs[0].d[14] & 1;
        }
        std::vector<uint8_t> held_next;
        if (paired == 1 && !last && (recs.size() & 1)) {
            held_next.assign(recs.back().d, recs.back().d + recs.back().n);
            recs.pop_back();
        }
        read_s += since(t0);
        t0 = std::chrono::steady_clock::now();
        F.extract(recs, pool, true, path);
        fields_s += since(t0);
        t0 = std::chrono::steady_clock::now();
        rsem_alncheck_verdict v;
        const int rc = rsem_alncheck_push(ck, (int64_t)recs.size(), F.name_off.data(), F.names.data(), F.flag.data(), F.tid.data(), F.pos.data(), F.isize.data(), F.lq.data(),
                                          F.cigar_off.data(), F.cigar.data(), last ? 1 : 0, &v);
        if (rc != RSEM_OK) die("%s: %s: %s (this program has no CPU path)", path.c_str(), rsem_hip_strerror(rc), rsem_hip_last_error());
        device_s += since(t0);
        records += recs.size(); pushes++; batches += (uint64_t)v.n_batches; launches += (uint64_t)v.n_launches; upload_ms += v.upload_ms; kernel_ms += v.kernel_ms;
        device_bytes = v.device_bytes; groups = v.resident_groups; name_bytes = v.resident_name_bytes;
        cnt += v.units_ok;
        for (; (dots + 1) * 1000000 <= cnt; dots++) { printf("."); fflush(stdout); }  // samValidator.cpp:181
        if (v.code) { print_verdict(v, recs, H); valid = false; }
        held.swap(held_next);
        t0 = std::chrono::steady_clock::now();
    }
    rsem_alncheck_destroy(ck);
    if (valid) printf("\nThe input file is valid!\n");
    else printf("The input file is not valid!\n");
    if (getenv("RSEM_HIP_TIMING"))
        printf("[timing] {\"wall_s\": %.4f, \"inflate_cut_s\": %.4f, \"fields_s\": %.4f, \"device_call_s\": %.4f, \"upload_ms\": %.3f, \"kernel_ms\": %.3f, \"threads\": %d, "
               "\"records\": %llu, \"units_ok\": %llu, \"groups\": %llu, \"name_bytes\": %llu, \"pushes\": %llu, \"batches\": %llu, \"launches\": %llu, \"device_bytes\": %llu}\n",
               since(t_all), read_s, fields_s, device_s, upload_ms, kernel_ms, nthreads, (unsigned long long)records, (unsigned long long)cnt, (unsigned long long)groups,
               (unsigned long long)name_bytes, (unsigned long long)pushes, (unsigned long long)batches, (unsigned long long)launches, (unsigned long long)device_bytes);
}

// ---- rsem-get-unique ---------------------------------------------------------------------------------------------------------------

// the header as bam_hdr_write writes what sam_hdr_read read: a BAM's own bytes (its text with whatever padding it has); a SAM's text
// and the dictionary of its @SQ lines
inline std::vector<uint8_t> header_bytes_as_read(const std::string& path, const AlignmentReader& in) {
    std::vector<uint8_t> raw;
    auto put = [&](const void* q, size_t n) { raw.insert(raw.end(), (const uint8_t*)q, (const uint8_t*)q + n); };
    if (in.is_bam()) {
        BgzfReader z;
        if (!z.open(path)) die("Cannot open %s!", path.c_str());
        raw.resize((size_t)in.records_at());
        if (!z.read(raw.data(), raw.size())) die("input BAM: the file ends inside its header");
        return raw;
    }
    const AlnHeader& H = in.header;
    put("BAM\1", 4);
    const int32_t l_text = (int32_t)H.text.size();
    put(&l_text, 4);
    put(H.text.data(), (size_t)l_text);
    const int32_t n_ref = (int32_t)H.names.size();
    put(&n_ref, 4);
    for (int i = 0; i < n_ref; i++) {
        const int32_t l_name = (int32_t)H.names[i].size() + 1;
        put(&l_name, 4);
        put(H.names[i].c_str(), (size_t)l_name);
        put(&H.lens[i], 4);
    }
    return raw;
}

inline void write_unique(const std::string& inF, const std::string& outF, const AlncheckOptions& opt) {
    const auto t_all = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    refuse_cram(inF);
    AlignmentReader in;
    in.open(inF);
    const int nthreads = pool_threads(opt.threads);
    StagePool pool(nthreads);
    std::vector<BgzfDeflater> defl((size_t)nthreads);
    FILE* fo = fopen(outF.c_str(), "wb");
    if (!fo) die("Cannot open %s for writing!", outF.c_str());
    uint64_t out_bytes = 0;
    {
        const std::vector<uint8_t> raw = header_bytes_as_read(inF, in);
        std::vector<uint8_t> comp;
        defl[0].stream(raw.data(), raw.size(), comp);
        if (fwrite(comp.data(), 1, comp.size(), fo) != comp.size()) die("Cannot write %s!", outF.c_str());
        out_bytes += comp.size();
    }
    size_t super_bytes = 64u << 20;
    if (const char* e = getenv("RSEM_HIP_BAM_CHUNK")) super_bytes = std::max<size_t>(64, (size_t)atoll(e));
    RecordChunks chunks(inF, in, pool, super_bytes);
    std::vector<RecView> fresh, recs;
    std::vector<std::vector<uint8_t>> held, held_next;  // the records of the group that the super-chunk's end may have cut
    RecordFields F;
    std::vector<uint8_t> keep;
    struct Piece { std::vector<uint8_t> out; };
    std::vector<Piece> pieces;
    double read_s = 0, fields_s = 0, device_s = 0, deflate_s = 0, write_s = 0, upload_ms = 0, kernel_ms = 0;
    uint64_t cnt = 0, dots = 0, kept = 0, groups = 0, calls = 0, batches = 0, device_bytes = 0;
    bool last = false;
    auto t0 = std::chrono::steady_clock::now();
    while (chunks.next(fresh, last)) {
        recs.clear();
        for (const auto& h : held) recs.push_back({h.data(), h.size()});
        recs.insert(recs.end(), fresh.begin(), fresh.end());
        for (const RecView& r : recs)
            if (r.n < 33) die("%s: an alignment record of fewer than 33 bytes", inF.c_str());
        size_t n = recs.size();
        if (!last && n) {  // the last group waits (getUnique.cpp:56: the raw names decide)
            size_t k = n - 1;
            while (k > 0) {
                const auto a = raw_name(recs[k]), b = raw_name(recs[k - 1]);
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
        F.extract(recs, pool, false, inF);
        fields_s += since(t0);
        t0 = std::chrono::steady_clock::now();
        keep.assign(n + 1, 0);
        rsem_alncheck_info info;
        memset(&info, 0, sizeof(info));
        const int rc = rsem_alncheck_unique(opt.device, (int64_t)n, F.name_off.data(), F.names.data(), F.flag.data(), keep.data(), &info);
        if (rc != RSEM_OK) die("%s: %s: %s (this program has no CPU path)", inF.c_str(), rsem_hip_strerror(rc), rsem_hip_last_error());
        device_s += since(t0);
        calls++; batches += (uint64_t)info.n_batches; upload_ms += info.upload_ms; kernel_ms += info.kernel_ms; groups += info.n_groups; kept += info.n_kept;
        device_bytes = std::max<uint64_t>(device_bytes, info.device_bytes);
        t0 = std::chrono::steady_clock::now();
        const size_t np = std::max<size_t>(1, std::min<size_t>((size_t)nthreads * 4, n / 1024 + 1));
        pieces.assign(np, Piece());
        pool.run(np, [&](size_t i, int me) {
            std::vector<uint8_t> raw;
            for (size_t r = n * i / np, e = n * (i + 1) / np; r < e; r++) {
                if (!keep[r]) continue;
                const int32_t bs = (int32_t)recs[r].n;
                raw.insert(raw.end(), (const uint8_t*)&bs, (const uint8_t*)&bs + 4);
                raw.insert(raw.end(), recs[r].d, recs[r].d + recs[r].n);
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
        cnt += n;
        for (; (dots + 1) * 1000000 <= cnt; dots++) { printf("."); fflush(stdout); }  // getUnique.cpp:68
        held.swap(held_next);
        t0 = std::chrono::steady_clock::now();
    }
    bgzf_write_eof(fo);
    if (fclose(fo) != 0) die("Cannot write %s!", outF.c_str());
    if (cnt >= 1000000) printf("\n");
    printf("done!\n");
    if (getenv("RSEM_HIP_TIMING"))
        printf("[timing] {\"wall_s\": %.4f, \"inflate_cut_s\": %.4f, \"fields_s\": %.4f, \"device_call_s\": %.4f, \"upload_ms\": %.3f, \"kernel_ms\": %.3f, \"deflate_s\": %.4f, "
               "\"write_s\": %.4f, \"threads\": %d, \"records\": %llu, \"groups\": %llu, \"kept\": %llu, \"device_calls\": %llu, \"batches\": %llu, \"device_bytes\": %llu, "
               "\"out_bytes\": %llu}\n",
               since(t_all), read_s, fields_s, device_s, upload_ms, kernel_ms, deflate_s, write_s, nthreads, (unsigned long long)cnt, (unsigned long long)groups,
               (unsigned long long)kept, (unsigned long long)calls, (unsigned long long)batches, (unsigned long long)device_bytes, (unsigned long long)out_bytes);
}

}  // namespace rsemh
