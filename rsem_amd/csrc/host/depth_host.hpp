// depth_host.hpp -- the host side of rsem-bam2wig and rsem-bam2readdepth (wiggle.cpp:16-139): alignment records -> blocks and runs,
// the device call (rsem_depth_accumulate, rsem_amd/csrc/depth.hip), the two writers.  DESIGN.md section 11.
//
// The reference reads record by record on one thread, adds `w` to read_depth[pos] once per base of every M block, and hands the
// array to its writer whenever core.tid differs from the previous counted record's.  A maximal stretch of consecutive mapped
// records with one tid is a RUN here; a tid that comes back is a second run and is written a second time, as there.
//
//   read     SAM text or BAM (AlignmentReader of bam_io.hpp; BGZF blocks inflated side by side), in super-chunks; the records of a
//            super-chunk are cut into pieces, and the threads turn every piece into blocks (position, length, weight) and the places
//            where the tid changes (add_record);
//   stitch   one thread walks the pieces in order: runs are laid one after the other in a coordinate space, blocks get their place in it;
//   device   when the space holds enough blocks, or the next run does not fit its base budget: depth[b] = the fold of the weights;
//   format   the finished runs' text, in pieces on the threads, written in order.  A run that is still open when the space is handed
//            over keeps its depth and goes on in the next space (the device call continues the fold from the values passed in).
#pragma once
#include <chrono>

#include "../../../include/rsem_hip.h"
#include "bam_io.hpp"

namespace rsemh {

// ---- records -> blocks --------------------------------------------------------------------------------------------------

struct DepthPiece {
    std::vector<uint32_t> pos, len;  // M blocks, in record order
    std::vector<double> w;
    struct Change { uint64_t block; int32_t tid; };  // from block `block` of the piece on, the records are of tid (the first counted record always says so)
    std::vector<Change> changes;
    uint64_t counted = 0;  // mapped records
    int32_t last_tid = -1;
    std::string error;     // the first record the program stops at
    void clear() { pos.clear(); len.clear(); w.clear(); changes.clear(); counted = 0; last_tid = -1; error.clear(); }
};

// bam_aux_get (htslib 1.3 sam.c:1240-1256): the type byte of the first field `a b` behind p, or NULL
inline const uint8_t* aux_find(const uint8_t* d, size_t n, size_t p, char a, char b) {
    while (p + 3 <= n) {
        if (d[p] == (uint8_t)a && d[p + 1] == (uint8_t)b) return d + p + 2;
        const char type = (char)d[p + 2];
        p += 3;
        switch (type) {
            case 'A': case 'c': case 'C': p += 1; break;
            case 's': case 'S': p += 2; break;
            case 'i': case 'I': case 'f': p += 4; break;
            case 'd': p += 8; break;
            case 'Z': case 'H': while (p < n && d[p]) ++p; ++p; break;
            case 'B': {
                if (p + 5 > n) return nullptr;
                const char sub = (char)d[p];
                int32_t cnt;
                memcpy(&cnt, d + p + 1, 4);
                const int sz = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                p += 5 + (size_t)(cnt < 0 ? 0 : cnt) * sz;
                break;
            }
            default: return nullptr;
        }
    }
    return nullptr;
}

// One BAM record (without its block_size word), as add_bam_record_to_wiggle and the loop around it see it (wiggle.cpp:16-37,54-66).
// Returns false where the program stops (P.error says why).
inline bool add_record(DepthPiece& P, const uint8_t* d, size_t n, const AlnHeader& H, bool no_fractional_weight) {
    if (n < 32) { P.error = "an alignment record of fewer than 32 bytes"; return false; }
    const uint16_t flag = (uint16_t)(d[14] | (d[15] << 8));
    if (flag & 4) return true;  // bam_is_unmapped: before the switch of sequence and the count
    int32_t tid, pos, l_seq;
    uint16_t n_cig;
    memcpy(&tid, d, 4);
    memcpy(&pos, d + 4, 4);
    memcpy(&n_cig, d + 12, 2);
    memcpy(&l_seq, d + 16, 4);
    const size_t l_name = d[8];
    auto where = [&]() {
        std::string s = "the alignment of read ";
        s.append((const char*)d + 32, l_name && 32 + l_name <= n ? l_name - 1 : 0);
        char t[96];
        snprintf(t, sizeof(t), " (reference sequence id %d, position %lld)", tid, (long long)pos + 1);
        return s + t;
    };
    if (tid < 0 || (size_t)tid >= H.lens.size()) { P.error = where() + " is mapped but names no reference sequence of the header"; return false; }
    if (pos < 0) { P.error = where() + " is mapped but has no position"; return false; }
    const size_t cig_at = 32 + l_name, aux_at = cig_at + 4 * (size_t)n_cig + ((size_t)l_seq + 1) / 2 + (size_t)l_seq;
    if (l_seq < 0 || aux_at > n) { P.error = where() + " is cut short"; return false; }
    if (P.counted == 0 || tid != P.last_tid) P.changes.push_back({P.pos.size(), tid});
    P.last_tid = tid;
    P.counted++;
    double w = 1.0;
    if (!no_fractional_weight) {
        const uint8_t* t = aux_find(d, n, aux_at, 'Z', 'W');
        if (!t) return true;
        if (*t == 'f' && t + 5 <= d + n) { float f; memcpy(&f, t + 1, 4); w = f; }  // bam_aux2f (sam.c:1292-1299)
        else if (*t == 'd' && t + 9 <= d + n) memcpy(&w, t + 1, 8);
        else w = 0.0;
    }
    const int64_t tlen = (uint32_t)H.lens[tid];
    int64_t p = pos;
    for (size_t i = 0; i < n_cig; i++) {
        uint32_t c;
        memcpy(&c, d + cig_at + 4 * i, 4);
        const uint32_t op = c & 15, oplen = c >> 4;
        if (op == 0) {  // BAM_CMATCH; = and X do not add
            if (p + (int64_t)oplen > tlen) {
                char t[128];
                snprintf(t, sizeof(t), ": %uM from position %lld on runs past the end of %s (%lld bases)", oplen, (long long)p + 1, H.names[tid].c_str(), (long long)tlen);
                P.error = where() + t;
                return false;
            }
            if (oplen) { P.pos.push_back((uint32_t)p); P.len.push_back(oplen); P.w.push_back(w); }
            p += oplen;
        } else if (op == 2 || op == 3 || op == 7 || op == 8) p += oplen;  // bam_cigar_type(op) & 2: D N = X
    }
    return true;
}

// ---- the writers --------------------------------------------------------------------------------------------------------------

struct DepthWriter {
    virtual ~DepthWriter() {}
    // the text of the bases [lo, hi) of a used sequence (d: its whole depth); the pieces of a sequence are written in order
    virtual void piece(std::string& out, const std::string& name, uint32_t length, const double* d, uint32_t lo, uint32_t hi) const = 0;
    virtual void unused(std::string& out, const std::string& name, uint32_t length) const = 0;
};

// UCSCWiggleTrackWriter::process (wiggle.cpp:97-121): maximal stretches of bases with depth >= 0.0095, "%.2f" a line
struct WigWriter : DepthWriter {
    static std::string header(const char* track_name) {
        return std::string("track type=wiggle_0 name=\"") + track_name + "\" description=\"" + track_name + "\" visibility=full\n";
    }
    void piece(std::string& out, const std::string& name, uint32_t, const double* d, uint32_t lo, uint32_t hi) const override {
        char t[kCellBuf];
        for (uint32_t i = lo; i < hi; i++) {
            if (!(d[i] >= 0.0095)) continue;
            if (i == 0 || !(d[i - 1] >= 0.0095)) {
                out.append("fixedStep chrom=").append(name).append(" start=");
                out.append(t, (size_t)snprintf(t, sizeof(t), "%d", (int)(i + 1)));
                out.append(" step=1\n");
            }
            const int k = snprintf(t, sizeof(t), "%.2f\n", d[i]);
            if (k < 0 || k >= kCellBuf) die("a depth of %d characters does not fit", k);
            out.append(t, (size_t)k);
        }
    }
    void unused(std::string&, const std::string&, uint32_t) const override {}
};

// ReadDepthWriter::process (wiggle.cpp:127-139): name, length, the values as `ostream << double` prints them
struct ReadDepthWriter : DepthWriter {
    static void head(std::string& out, const std::string& name, uint32_t length) {
        char t[32];
        out.append(name).push_back('\t');
        out.append(t, (size_t)snprintf(t, sizeof(t), "%u\t", length));
    }
    void piece(std::string& out, const std::string& name, uint32_t length, const double* d, uint32_t lo, uint32_t hi) const override {
        if (lo == 0) head(out, name, length);
        if (length == 0) { out.append("NA\n"); return; }  // (read_depth.empty(): a used sequence of no bases)
        char t[48];
        for (uint32_t i = lo; i < hi; i++) {
            if (i > 0) out.push_back(' ');
            if (d[i] == 0.0 && !std::signbit(d[i])) out.push_back('0');
            else out.append(t, (size_t)snprintf(t, sizeof(t), "%g", d[i]));
        }
        if (hi == length) out.push_back('\n');
    }
    void unused(std::string& out, const std::string& name, uint32_t length) const override {
        head(out, name, length);
        out.append("NA\n");
    }
};

// ---- the pass -------------------------------------------------------------------------------------------------------------------

struct DepthOptions {
    bool no_fractional_weight = false, quiet = false;
    int threads = 1, device = 0;
};

struct DepthStats {
    double read_s = 0, stitch_s = 0, device_s = 0, format_s = 0, write_s = 0, upload_ms = 0, kernel_ms = 0;
    uint64_t records = 0, blocks = 0, entries = 0, tiles = 0, runs = 0, calls = 0, batches = 0, out_bytes = 0;
};

class DepthPass {
   public:
    DepthPass(const AlnHeader& H, const DepthOptions& opt, const DepthWriter& wr, FILE* fo, const std::string& in_name, const std::string& out_name,
              StagePool& pool)
        : H_(H), opt_(opt), wr_(wr), fo_(fo), in_name_(in_name), out_name_(out_name), pool_(pool), used_(H.names.size(), 0) {
        // test knobs: the results do not depend on them
        if (const char* e = getenv("RSEM_DEPTH_SPACE_BASES")) space_bases_max_ = std::max<uint64_t>(1, (uint64_t)atoll(e));
        if (const char* e = getenv("RSEM_DEPTH_SPACE_BLOCKS")) space_blocks_max_ = std::max<uint64_t>(1, (uint64_t)atoll(e));
    }
    DepthStats stats;

    // the pieces of a super-chunk, in order
    void stitch(std::vector<DepthPiece>& pieces) {
        const auto t0 = now();
        for (DepthPiece& P : pieces) {
            for (size_t c = 0; c < P.changes.size(); c++) {
                const uint64_t b0 = P.changes[c].block, b1 = c + 1 < P.changes.size() ? P.changes[c + 1].block : P.pos.size();
                if (P.changes[c].tid != cur_tid_) open_run(P.changes[c].tid);
                const uint64_t off = runs_.back().off;
                for (uint64_t b = b0; b < b1; b++) start_.push_back(off + P.pos[b]);
                len_.insert(len_.end(), P.len.begin() + b0, P.len.begin() + b1);
                w_.insert(w_.end(), P.w.begin() + b0, P.w.begin() + b1);
            }
            if (!P.error.empty()) die("%s: %s", in_name_.c_str(), P.error.c_str());
            const uint64_t before = stats.records;
            stats.records += P.counted;
            if (!opt_.quiet)
                for (uint64_t m = before / 1000000 + 1; m * 1000000 <= stats.records; m++) printf("%llu\n", (unsigned long long)(m * 1000000));  // wiggle.cpp:66
        }
        stats.stitch_s += since(t0);
        if (start_.size() >= space_blocks_max_) hand_over(true);
    }
    void finish() {
        hand_over(false);
        std::string out;
        for (size_t i = 0; i < H_.names.size(); i++)  // wiggle.cpp:70-76
            if (!used_[i]) wr_.unused(out, H_.names[i], (uint32_t)H_.lens[i]);
        write(out);
    }

   private:
    struct Run { int32_t tid; uint64_t off; uint32_t len; };
    const AlnHeader& H_;
    const DepthOptions& opt_;
    const DepthWriter& wr_;
    FILE* fo_;
    std::string in_name_, out_name_;
    StagePool& pool_;
    std::vector<char> used_;
    std::vector<Run> runs_;
    std::vector<uint64_t> start_;
    std::vector<uint32_t> len_;
    std::vector<double> w_, depth_;
    uint64_t space_bases_ = 0, space_bases_max_ = 1ull << 27, space_blocks_max_ = 1ull << 24;
    int32_t cur_tid_ = -1;

    static std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
    static double since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); }
    void write(const std::string& s) {
        const auto t0 = now();
        if (!s.empty() && fwrite(s.data(), 1, s.size(), fo_) != s.size()) die("Cannot write %s!", out_name_.c_str());
        stats.out_bytes += s.size();
        stats.write_s += since(t0);
    }
    void open_run(int32_t tid) {
        const uint32_t len = (uint32_t)H_.lens[tid];
        if (!runs_.empty() && space_bases_ + len > space_bases_max_) hand_over(false);  // (every run of the space is finished here)
        runs_.push_back({tid, space_bases_, len});
        space_bases_ += len;
        depth_.resize(space_bases_, 0.0);
        used_[tid] = 1;
        cur_tid_ = tid;
        stats.runs++;
    }
    // the space goes to the device; the finished runs are written; with keep_open the last run goes on in the next space
    void hand_over(bool keep_open) {
        if (runs_.empty()) return;
        auto t0 = now();
        rsem_depth_info info;
        memset(&info, 0, sizeof(info));
        const int rc = rsem_depth_accumulate(opt_.device, space_bases_, start_.size(), start_.data(), len_.data(), w_.data(), depth_.data(), &info);
        if (rc != RSEM_OK) die("%s: %s: %s (this program has no CPU path)", in_name_.c_str(), rsem_hip_strerror(rc), rsem_hip_last_error());
        stats.device_s += since(t0);
        stats.calls++;
        stats.blocks += start_.size();
        stats.entries += info.n_entries;
        stats.tiles += info.n_tiles_touched;
        stats.batches += (uint64_t)info.n_batches;
        stats.upload_ms += info.upload_ms;
        stats.kernel_ms += info.kernel_ms;
        start_.clear(); len_.clear(); w_.clear();

        // the finished runs' text: items of at most 64 K bases, a group of them at a time on the threads, written in order
        const size_t n_done = runs_.size() - (keep_open ? 1 : 0);
        struct Item { size_t run; uint32_t lo, hi; };
        std::vector<Item> items;
        const size_t group = (size_t)pool_.threads() * 4;
        std::vector<std::string> text(group);
        auto flush_items = [&]() {
            t0 = now();
            pool_.run(items.size(), [&](size_t i, int) {
                const Run& R = runs_[items[i].run];
                text[i].clear();
                wr_.piece(text[i], H_.names[R.tid], R.len, depth_.data() + R.off, items[i].lo, items[i].hi);
            });
            stats.format_s += since(t0);
            for (size_t i = 0; i < items.size(); i++) write(text[i]);
            items.clear();
        };
        for (size_t r = 0; r < n_done; r++) {
            const uint32_t len = runs_[r].len;
            for (uint32_t lo = 0;;) {
                const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)lo + 65536, len);
                items.push_back({r, lo, hi});
                if (items.size() == group) flush_items();
                if (hi >= len) break;
                lo = hi;
            }
        }
        flush_items();
        if (keep_open) {
            const Run last = runs_.back();
            memmove(depth_.data(), depth_.data() + last.off, (size_t)last.len * 8);
            runs_.assign(1, Run{last.tid, 0, last.len});
            space_bases_ = last.len;
        } else {
            runs_.clear();
            space_bases_ = 0;
        }
        depth_.resize(space_bases_);
    }
};

// build_wiggles (wiggle.cpp:39-83) for either program.  `fo` is the open output file (the reference opens it before the input).
inline void build_depth(const std::string& path, const DepthOptions& opt, const DepthWriter& wr, FILE* fo, const std::string& out_name) {
    const auto t_all = std::chrono::steady_clock::now();
    {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) die("Cannot open %s!", path.c_str());
        char magic[4] = {0, 0, 0, 0};
        const size_t got = fread(magic, 1, 4, f);
        fclose(f);
        if (got == 4 && !memcmp(magic, "CRAM", 4)) die("%s is a CRAM file: CRAM input is not supported, convert it to BAM first (samtools view -b)", path.c_str());
    }
    AlignmentReader in;
    in.open(path);
    const AlnHeader& H = in.header;
    int nthreads = std::max(1, std::min(opt.threads, (int)std::max(1u, std::thread::hardware_concurrency())));
    if (const int granted = cgroup_cpu_cores()) nthreads = std::max(1, std::min(nthreads, granted));
    StagePool pool(nthreads);
    DepthPass pass(H, opt, wr, fo, path, out_name, pool);
    size_t super_bytes = 64u << 20;
    if (const char* e = getenv("RSEM_HIP_BAM_CHUNK")) super_bytes = std::max<size_t>(64, (size_t)atoll(e));
    const size_t n_pieces_max = (size_t)nthreads * 4;
    std::vector<DepthPiece> pieces;
    double read_s = 0;
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };

    if (!in.is_bam()) {
        const char* cur = in.body_begin();
        const char* const end = in.body_end();
        while (cur < end) {
            const auto t0 = std::chrono::steady_clock::now();
            const char* sc_end = cur + std::min<size_t>(super_bytes, (size_t)(end - cur));
            if (sc_end < end) {
                const char* nl = (const char*)memchr(sc_end, '\n', end - sc_end);
                sc_end = nl ? nl + 1 : end;
            }
            const std::vector<size_t> cut = line_chunks(cur, 0, (size_t)(sc_end - cur), (int)std::min<size_t>(n_pieces_max, (size_t)(sc_end - cur) / 4096 + 1));
            pieces.resize(cut.size() - 1);
            pool.run(pieces.size(), [&](size_t i, int) {
                DepthPiece& P = pieces[i];
                P.clear();
                AlnRecord r;
                for (const char *q = cur + cut[i], *lim = cur + cut[i + 1]; q < lim;) {
                    const char* nl = (const char*)memchr(q, '\n', lim - q);
                    const char* e = nl ? nl : lim;
                    const char* next = nl ? nl + 1 : lim;
                    if (e > q && e[-1] == '\r') --e;
                    if (e > q) {
                        in.encode_sam_line(q, e, r);
                        if (!add_record(P, r.d.data(), r.d.size(), H, opt.no_fractional_weight)) break;
                    }
                    q = next;
                }
            });
            read_s += since(t0);
            pass.stitch(pieces);
            cur = sc_end;
        }
    } else {
        MappedFile mf;
        if (!mf.open(path)) die("Cannot open %s!", path.c_str());
        struct Blk { size_t off, clen; uint32_t isize, crc; };
        std::vector<Blk> blks;
        for (size_t o = 0; o + 18 <= mf.size;) {
            const uint8_t* h = (const uint8_t*)mf.data + o;
            if (h[0] != 0x1f || h[1] != 0x8b || !(h[3] & 4)) die("input BAM: not a BGZF block");
            const int xlen = h[10] | (h[11] << 8);
            int bsize = -1;
            for (int i = 0; i + 4 <= xlen && o + 12 + (size_t)i + 6 <= mf.size;) {
                const uint8_t* x = h + 12 + i;
                const int slen = x[2] | (x[3] << 8);
                if (x[0] == 'B' && x[1] == 'C' && slen == 2) bsize = x[4] | (x[5] << 8);
                i += 4 + slen;
            }
            if (bsize < 12 + xlen + 8 - 1 || o + (size_t)bsize + 1 > mf.size) die("input BAM: truncated or corrupt BGZF block");
            uint32_t isize, crc;
            memcpy(&isize, h + bsize + 1 - 4, 4);
            memcpy(&crc, h + bsize + 1 - 8, 4);
            if (isize > 0x10000) die("input BAM: a BGZF block of more than 64 KiB");
            blks.push_back({o + 12 + (size_t)xlen, (size_t)bsize + 1 - 12 - xlen - 8, isize, crc});
            o += (size_t)bsize + 1;
        }
        std::vector<uint8_t> buf, carry;
        std::vector<uint64_t> rec;
        uint64_t skip = in.records_at();  // header bytes of the uncompressed stream still to pass
        for (size_t bi = 0; bi < blks.size();) {
            const auto t0 = std::chrono::steady_clock::now();
            size_t be = bi, bytes = 0;
            while (be < blks.size() && (be == bi || bytes + blks[be].isize <= super_bytes)) bytes += blks[be++].isize;
            std::vector<size_t> at(be - bi + 1, carry.size());
            for (size_t k = bi; k < be; k++) at[k - bi + 1] = at[k - bi] + blks[k].isize;
            buf.resize(at.back());
            if (!carry.empty()) memcpy(buf.data(), carry.data(), carry.size());
            pool.run(be - bi, [&](size_t k, int) {
                const Blk& B = blks[bi + k];
                if (!B.isize) return;
                // this repository's decoder first, believed only if the block's own CRC-32 agrees; anything else goes to zlib
                static thread_local std::unique_ptr<FastInflate> fi;
                if (!fi) fi.reset(new FastInflate());
                uint8_t* dst = buf.data() + at[k];
                if (fi->inflate((const uint8_t*)mf.data + B.off, B.clen, dst, B.isize) && crc32_fast(0u, dst, B.isize) == B.crc) return;
                z_stream zs;
                memset(&zs, 0, sizeof(zs));
                if (inflateInit2(&zs, -15) != Z_OK) die("zlib inflateInit2 failed");
                zs.next_in = (Bytef*)mf.data + B.off; zs.avail_in = (uInt)B.clen;
                zs.next_out = dst; zs.avail_out = B.isize;
                const int rc = inflate(&zs, Z_FINISH);
                inflateEnd(&zs);
                if (rc != Z_STREAM_END) die("input BAM: corrupt BGZF block");
                if (crc32_fast(0u, dst, B.isize) != B.crc) die("input BAM: a BGZF block's checksum does not match its data");
            });
            bi = be;
            // frame: the records that are complete in the buffer; what is left over waits for the next super-chunk
            const size_t n = buf.size();
            size_t pos = 0;
            if (skip) { const size_t k = (size_t)std::min<uint64_t>(skip, n); pos = k; skip -= k; }
            rec.clear();
            while (pos + 4 <= n) {
                int32_t bs;
                memcpy(&bs, buf.data() + pos, 4);
                if (bs < 32) die("input BAM: corrupt alignment record");
                if (pos + 4 + (size_t)bs > n) break;
                rec.push_back(pos);
                pos += 4 + (size_t)bs;
            }
            if (bi >= blks.size() && pos != n) die("input BAM: the last record is cut short");
            carry.assign(buf.begin() + pos, buf.end());
            const size_t np = std::max<size_t>(1, std::min(n_pieces_max, rec.size() / 64 + 1));
            pieces.resize(np);
            pool.run(np, [&](size_t i, int) {
                DepthPiece& P = pieces[i];
                P.clear();
                for (size_t r = rec.size() * i / np, re = rec.size() * (i + 1) / np; r < re; r++) {
                    int32_t bs;
                    memcpy(&bs, buf.data() + rec[r], 4);
                    if (!add_record(P, buf.data() + rec[r] + 4, (size_t)bs, H, opt.no_fractional_weight)) break;
                }
            });
            read_s += since(t0);
            pass.stitch(pieces);
        }
        if (skip) die("input BAM: the file ends inside its header");
    }
    pass.finish();
    if (getenv("RSEM_HIP_TIMING")) {
        const DepthStats& s = pass.stats;
        printf("[timing] {\"wall_s\": %.4f, \"read_blocks_s\": %.4f, \"stitch_s\": %.4f, \"device_call_s\": %.4f, \"upload_ms\": %.3f, \"kernel_ms\": %.3f, "
               "\"format_s\": %.4f, \"write_s\": %.4f, \"threads\": %d, \"records\": %llu, \"blocks\": %llu, \"entries\": %llu, \"tiles_touched\": %llu, "
               "\"runs\": %llu, \"device_calls\": %llu, \"batches\": %llu, \"out_bytes\": %llu}\n",
               since(t_all), read_s, s.stitch_s, s.device_s, s.upload_ms, s.kernel_ms, s.format_s, s.write_s, nthreads, (unsigned long long)s.records,
               (unsigned long long)s.blocks, (unsigned long long)s.entries, (unsigned long long)s.tiles, (unsigned long long)s.runs,
               (unsigned long long)s.calls, (unsigned long long)s.batches, (unsigned long long)s.out_bytes);
    }
}

// the options both programs take behind the reference's arguments: -p N, --device N, -q.  Returns false on anything else.
inline bool parse_depth_options(int argc, char* argv[], int from, DepthOptions& opt) {
    for (int i = from; i < argc; i++) {
        if (!strcmp(argv[i], "-q")) opt.quiet = true;
        else if (!strcmp(argv[i], "-p") && i + 1 < argc) opt.threads = std::max(1, atoi(argv[++i]));
        else if (!strcmp(argv[i], "--device") && i + 1 < argc) opt.device = atoi(argv[++i]);
        else return false;
    }
    return true;
}

}  // namespace rsemh
