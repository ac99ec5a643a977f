// gbam_host.hpp -- the host side of rsem-tbam2gbam (tbam2gbam.cpp, BamConverter.h, bc_aux.h, SamHeader.cpp): header, records ->
// fields, the device call (rsem_gmap_convert, rsem_amd/csrc/gmap.hip), fields -> records, BGZF out.  DESIGN.md section 12.
//
// The reference reads, converts, collapses and writes record by record on one thread (htslib's -p threads only deflate).  Here
//   read      SAM text or BAM (AlignmentReader of bam_io.hpp; BGZF blocks inflated side by side), in super-chunks;
//   cut       records -> units (a record, or a pair of mates) -> groups (the consecutive mapped units of one read name); a group that
//             the super-chunk's end may cut is held back for the next one;
//   fields    per mate transcript, pos, l_qseq, flag, per alignment the ZW weight -- on the -p threads;
//   device    rsem_gmap_convert: per mate tid, pos, flag, bin, CIGAR; per group which alignments stay, in which order, their weights;
//   assemble  the output records from the input records' bytes and the returned fields (qname, new CIGAR, SEQ and QUAL flipped while
//             they are copied, MD reversed, XS removed or appended, ZW and MAPQ), deflated piece by piece -- on the -p threads;
//   write     the pieces' block runs in order.
#pragma once
#include <chrono>

#include "../../../include/rsem_hip.h"
#include "bam_io.hpp"

namespace rsemh {

struct GbamOptions {
    bool quiet = false;
    int threads = 1, device = 0;
};

struct RecView { const uint8_t* d; size_t n; };

// ---- super-chunks of records ------------------------------------------------------------------------------------------------------

class RecordChunks {
   public:
    RecordChunks(const std::string& path, AlignmentReader& in, StagePool& pool, size_t super_bytes) : path_(path), in_(in), pool_(pool), super_(super_bytes) {
        if (in_.is_bam()) {
            if (!mf_.open(path)) die("Cannot open %s!", path.c_str());
            for (size_t o = 0; o + 18 <= mf_.size;) {
                const uint8_t* h = (const uint8_t*)mf_.data + o;
                if (h[0] != 0x1f || h[1] != 0x8b || !(h[3] & 4)) die("input BAM: not a BGZF block");
                const int xlen = h[10] | (h[11] << 8);
                int bsize = -1;
                for (int i = 0; i + 4 <= xlen && o + 12 + (size_t)i + 6 <= mf_.size;) {
                    const uint8_t* x = h + 12 + i;
                    const int slen = x[2] | (x[3] << 8);
                    if (x[0] == 'B' && x[1] == 'C' && slen == 2) bsize = x[4] | (x[5] << 8);
                    i += 4 + slen;
                }
                if (bsize < 12 + xlen + 8 - 1 || o + (size_t)bsize + 1 > mf_.size) die("input BAM: truncated or corrupt BGZF block");
                uint32_t isize, crc;
                memcpy(&isize, h + bsize + 1 - 4, 4);
                memcpy(&crc, h + bsize + 1 - 8, 4);
                if (isize > 0x10000) die("input BAM: a BGZF block of more than 64 KiB");
                blks_.push_back({o + 12 + (size_t)xlen, (size_t)bsize + 1 - 12 - xlen - 8, isize, crc});
                o += (size_t)bsize + 1;
            }
            skip_ = in_.records_at();
        } else {
            cur_ = in_.body_begin();
            end_ = in_.body_end();
        }
    }
    // the records of the next super-chunk (views that stay until the call after); false when the file is through
    bool next(std::vector<RecView>& recs, bool& last) {
        recs.clear();
        return in_.is_bam() ? next_bam(recs, last) : next_sam(recs, last);
    }

   private:
    struct Blk { size_t off, clen; uint32_t isize, crc; };
    struct SamPiece { std::vector<uint8_t> buf; std::vector<size_t> at; };
    std::string path_;
    AlignmentReader& in_;
    StagePool& pool_;
    size_t super_;
    MappedFile mf_;
    std::vector<Blk> blks_;
    size_t bi_ = 0;
    uint64_t skip_ = 0;
    std::vector<uint8_t> buf_, carry_;
    const char *cur_ = nullptr, *end_ = nullptr;
    std::vector<SamPiece> sam_;

    bool next_sam(std::vector<RecView>& recs, bool& last) {
        if (cur_ >= end_) return false;
        const char* sc_end = cur_ + std::min<size_t>(super_, (size_t)(end_ - cur_));
        if (sc_end < end_) {
            const char* nl = (const char*)memchr(sc_end, '\n', end_ - sc_end);
            sc_end = nl ? nl + 1 : end_;
        }
        const std::vector<size_t> cut = line_chunks(cur_, 0, (size_t)(sc_end - cur_), (int)std::min<size_t>((size_t)pool_.threads() * 4, (size_t)(sc_end - cur_) / 4096 + 1));
        sam_.resize(cut.size() - 1);
        const char* base = cur_;
        pool_.run(sam_.size(), [&](size_t i, int) {
            SamPiece& P = sam_[i];
            P.buf.clear(); P.at.clear();
            AlnRecord r;
            for (const char *q = base + cut[i], *lim = base + cut[i + 1]; q < lim;) {
                const char* nl = (const char*)memchr(q, '\n', lim - q);
                const char* e = nl ? nl : lim;
                const char* nx = nl ? nl + 1 : lim;
                if (e > q && e[-1] == '\r') --e;
                if (e > q) {
                    in_.encode_sam_line(q, e, r);
                    P.at.push_back(P.buf.size());
                    P.buf.insert(P.buf.end(), r.d.begin(), r.d.end());
                }
                q = nx;
            }
            P.at.push_back(P.buf.size());
        });
        for (const SamPiece& P : sam_)
            for (size_t k = 0; k + 1 < P.at.size(); k++) recs.push_back({P.buf.data() + P.at[k], P.at[k + 1] - P.at[k]});
        cur_ = sc_end;
        last = cur_ >= end_;
        return true;
    }
    bool next_bam(std::vector<RecView>& recs, bool& last) {
        if (bi_ >= blks_.size()) {
            if (skip_) die("input BAM: the file ends inside its header");
            return false;
        }
        size_t be = bi_, bytes = 0;
        while (be < blks_.size() && (be == bi_ || bytes + blks_[be].isize <= super_)) bytes += blks_[be++].isize;
        std::vector<size_t> at(be - bi_ + 1, carry_.size());
        for (size_t k = bi_; k < be; k++) at[k - bi_ + 1] = at[k - bi_] + blks_[k].isize;
        buf_.resize(at.back());
        if (!carry_.empty()) memcpy(buf_.data(), carry_.data(), carry_.size());
        const size_t b0 = bi_;
        pool_.run(be - bi_, [&](size_t k, int) {
            const Blk& B = blks_[b0 + k];
            if (!B.isize) return;
            // this repository's decoder first, believed only if the block's own CRC-32 agrees; anything else goes to zlib
            static thread_local std::unique_ptr<FastInflate> fi;
            if (!fi) fi.reset(new FastInflate());
            uint8_t* dst = buf_.data() + at[k];
            if (fi->inflate((const uint8_t*)mf_.data + B.off, B.clen, dst, B.isize) && crc32_fast(0u, dst, B.isize) == B.crc) return;
            z_stream zs;
            memset(&zs, 0, sizeof(zs));
            if (inflateInit2(&zs, -15) != Z_OK) die("zlib inflateInit2 failed");
            zs.next_in = (Bytef*)mf_.data + B.off; zs.avail_in = (uInt)B.clen;
            zs.next_out = dst; zs.avail_out = B.isize;
            const int rc = inflate(&zs, Z_FINISH);
            inflateEnd(&zs);
            if (rc != Z_STREAM_END) die("input BAM: corrupt BGZF block");
            if (crc32_fast(0u, dst, B.isize) != B.crc) die("input BAM: a BGZF block's checksum does not match its data");
        });
        bi_ = be;
        const size_t n = buf_.size();
        size_t pos = 0;
        if (skip_) { const size_t k = (size_t)std::min<uint64_t>(skip_, n); pos = k; skip_ -= k; }
        while (pos + 4 <= n) {
            int32_t bs;
            memcpy(&bs, buf_.data() + pos, 4);
            if (bs < 32) die("input BAM: corrupt alignment record");
            if (pos + 4 + (size_t)bs > n) break;
            recs.push_back({buf_.data() + pos + 4, (size_t)bs});
            pos += 4 + (size_t)bs;
        }
        last = bi_ >= blks_.size();
        if (last && pos != n) die("input BAM: the last record is cut short");
        carry_.assign(buf_.begin() + pos, buf_.end());
        return true;
    }
};

// ---- a record's parts -------------------------------------------------------------------------------------------------------------

struct RecCore {
    int32_t tid, pos, l_seq, mtid, mpos, isize;
    uint32_t l_name, n_cigar, flag;
    size_t seq_at, qual_at, aux_at;
};

inline bool rec_core(const RecView& r, RecCore& c) {
    if (r.n < 32) return false;
    const uint8_t* d = r.d;
    uint16_t nc, fl;
    memcpy(&c.tid, d, 4); memcpy(&c.pos, d + 4, 4);
    c.l_name = d[8];
    memcpy(&nc, d + 12, 2); memcpy(&fl, d + 14, 2);
    c.n_cigar = nc; c.flag = fl;
    memcpy(&c.l_seq, d + 16, 4); memcpy(&c.mtid, d + 20, 4); memcpy(&c.mpos, d + 24, 4); memcpy(&c.isize, d + 28, 4);
    if (c.l_seq < 0 || c.l_name < 1) return false;
    c.seq_at = 32 + (size_t)c.l_name + 4 * (size_t)c.n_cigar;
    c.qual_at = c.seq_at + ((size_t)c.l_seq + 1) / 2;
    c.aux_at = c.qual_at + (size_t)c.l_seq;
    return c.aux_at <= r.n;
}

// bam_get_canonical_name (sam_utils.h:54-61): the first whitespace-delimited word of the name
inline std::pair<const char*, size_t> canonical_name(const RecView& r) {
    const char* q = (const char*)r.d + 32;
    const size_t cap = r.n > 32 ? std::min<size_t>(r.d[8], r.n - 32) : 0;
    size_t k = 0;
    while (k < cap && q[k] && !strchr(" \t\n\r\f\v", q[k])) k++;
    return {q, k};
}

// one field of the auxiliary area: where it ends, or 0 where the area is broken
inline size_t aux_end(const uint8_t* d, size_t n, size_t p) {
    if (p + 3 > n) return 0;
    const char type = (char)d[p + 2];
    p += 3;
    switch (type) {
        case 'A': case 'c': case 'C': p += 1; break;
        case 's': case 'S': p += 2; break;
        case 'i': case 'I': case 'f': p += 4; break;
        case 'd': p += 8; break;
        case 'Z': case 'H': while (p < n && d[p]) ++p; ++p; break;
        case 'B': {
            if (p + 5 > n) return 0;
            const char sub = (char)d[p];
            int32_t cnt;
            memcpy(&cnt, d + p + 1, 4);
            const int sz = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            p += 5 + (size_t)(cnt < 0 ? 0 : cnt) * sz;
            break;
        }
        default: return 0;
    }
    return p <= n ? p : 0;
}

// (float)bam_aux2f of the first ZW (htslib 1.3 sam.c:1292-1299): f itself, d narrowed, another type 0; without the tag 1 (BamConverter.h:126-127)
inline float zw_weight(const RecView& r, size_t aux_at) {
    for (size_t p = aux_at; p + 3 <= r.n;) {
        const size_t e = aux_end(r.d, r.n, p);
        if (!e) break;
        if (r.d[p] == 'Z' && r.d[p + 1] == 'W') {
            if (r.d[p + 2] == 'f') { float f; memcpy(&f, r.d + p + 3, 4); return f; }
            if (r.d[p + 2] == 'd') { double x; memcpy(&x, r.d + p + 3, 8); return (float)x; }
            return 0.0f;
        }
        p = e;
    }
    return 1.0f;
}

// the MD string of a '-' transcript (BamConverter.h:255-293): the runs of digits and of other characters in reverse order; a run of
// digits as it is; another run reversed with A, C, G, T complemented, a leading ^ staying in front
inline void flip_md(uint8_t* s, size_t len) {
    std::string out;
    out.reserve(len);
    size_t e = len;
    while (e > 0) {
        size_t b = e - 1;
        const bool dig = s[b] >= '0' && s[b] <= '9';
        while (b > 0 && ((s[b - 1] >= '0' && s[b - 1] <= '9') == dig)) --b;
        if (dig) out.append((const char*)s + b, e - b);
        else {
            size_t from = b;
            if (s[b] == '^') { out.push_back('^'); from = b + 1; }
            for (size_t j = e; j > from; j--) {
                const char ch = (char)s[j - 1];
                out.push_back(ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : ch);
            }
        }
        e = b;
    }
    memcpy(s, out.data(), len);
}

// what the device returned for a mate, and what the host knows
struct MateOut {
    int32_t tid, pos, mate_pos;
    uint32_t flag, n_cigar, bin, has_n;
    const uint32_t* cigar;
    bool minus, paired;
};

// One output record (behind its block_size word) appended to `raw`: convert + modifyTags of BamConverter.h:150-191,251-303 as a copy.
// Returns where the record starts in raw; zw_at = offset (in raw) of the first ZW's payload, 0 without one.
inline size_t assemble_record(std::vector<uint8_t>& raw, const RecView& r, const RecCore& c, const MateOut& m, size_t& zw_at) {
    const size_t at = raw.size();
    const size_t n_out = 32 + c.l_name + 4 * (size_t)m.n_cigar + (c.qual_at - c.seq_at) + (size_t)c.l_seq + (r.n - c.aux_at) + 4;
    raw.resize(at + 4 + n_out);
    uint8_t* o = raw.data() + at + 4;
    auto w32 = [&](size_t off, int32_t v) { memcpy(o + off, &v, 4); };
    auto w16 = [&](size_t off, uint16_t v) { memcpy(o + off, &v, 2); };
    w32(0, m.tid); w32(4, m.pos);
    o[8] = (uint8_t)c.l_name; o[9] = 255;
    w16(10, (uint16_t)m.bin); w16(12, (uint16_t)m.n_cigar); w16(14, (uint16_t)m.flag);
    w32(16, c.l_seq);
    w32(20, m.paired ? m.tid : c.mtid);
    w32(24, m.paired ? m.mate_pos : c.mpos);
    w32(28, (m.minus && m.paired) ? (int32_t)(0u - (uint32_t)c.isize) : c.isize);
    size_t p = 32;
    memcpy(o + p, r.d + 32, c.l_name); p += c.l_name;
    memcpy(o + p, m.cigar, 4 * (size_t)m.n_cigar); p += 4 * (size_t)m.n_cigar;
    const uint8_t *seq = r.d + c.seq_at, *qual = r.d + c.qual_at;
    const int L = c.l_seq;
    if (!m.minus) {
        memcpy(o + p, seq, c.aux_at - c.seq_at);
        p += c.aux_at - c.seq_at;
    } else {
        static const uint8_t comp[16] = {0, 8, 4, 0, 2, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 15};
        for (int i = 0; i < L; i += 2) {  // flipSeq: nibble i of the output is the complement of nibble L - 1 - i
            const int a = L - 1 - i, b = L - 2 - i;
            const uint8_t na = (seq[a >> 1] >> ((~a & 1) << 2)) & 15, nb = b >= 0 ? (seq[b >> 1] >> ((~b & 1) << 2)) & 15 : 0;
            if (!comp[na] || (b >= 0 && !comp[nb]))
                die("Read %s: SEQ holds a base other than A, C, G, T and N, which cannot be reverse-complemented (the reference asserts here)", (const char*)r.d + 32);
            o[p++] = (uint8_t)(comp[na] << 4 | (b >= 0 ? comp[nb] : 0));
        }
        for (int i = 0; i < L; i++) o[p++] = qual[L - 1 - i];
    }
    // the tags: MD reversed on '-', the first XS left out, XS:A appended where the CIGAR has an N
    const size_t aux0 = p;
    bool md_done = false, xs_done = false;
    for (size_t q = c.aux_at; q < r.n;) {
        size_t e = aux_end(r.d, r.n, q);
        if (!e) e = r.n;  // (what cannot be walked is copied as it is)
        if (!xs_done && e - q >= 3 && r.d[q] == 'X' && r.d[q + 1] == 'S') { xs_done = true; q = e; continue; }
        memcpy(o + p, r.d + q, e - q);
        if (m.minus && !md_done && e - q >= 3 && r.d[q] == 'M' && r.d[q + 1] == 'D') {
            md_done = true;
            if (r.d[q + 2] == 'Z' && e - q >= 4) flip_md(o + p + 3, e - q - 4);
        }
        p += e - q;
        q = e;
    }
    if (m.has_n) { o[p++] = 'X'; o[p++] = 'S'; o[p++] = 'A'; o[p++] = m.minus ? '-' : '+'; }
    const int32_t bs = (int32_t)(p);
    memcpy(raw.data() + at, &bs, 4);
    raw.resize(at + 4 + p);
    zw_at = 0;
    for (size_t q = aux0; q + 3 <= p;) {
        const size_t e = aux_end(o, p, q);
        if (!e) break;
        if (o[q] == 'Z' && o[q + 1] == 'W') { zw_at = at + 4 + q + 3; break; }
        q = e;
    }
    return at;
}

// writeCollapsedLines (BamConverter.h:201-212): the four bytes of the float over the ZW's payload, whatever its type (what would fall
// behind the record is not written)
inline void put_weight(std::vector<uint8_t>& raw, size_t zw_at, float w) {
    const size_t k = std::min<size_t>(4, raw.size() - zw_at);
    memcpy(raw.data() + zw_at, &w, k);
}

// ---- the pass -------------------------------------------------------------------------------------------------------------------

struct GbamStats {
    double read_s = 0, cut_s = 0, fields_s = 0, device_s = 0, assemble_s = 0, deflate_s = 0, write_s = 0, upload_ms = 0, kernel_ms = 0;
    uint64_t records = 0, groups = 0, aln_in = 0, aln_out = 0, cigar_words = 0, calls = 0, batches = 0, out_bytes = 0;
};

// SamHeader (SamHeader.cpp:32-46,70-111, SamHeader.hpp:39-61): the lines regrouped, @SQ from the .chrlist, @PG ID:rsem-tbam2gbam
inline std::string genome_header_text(const std::string& text, const std::string& chrlist, const std::string& command) {
    std::string HD, SQ, RG, PG, CO, other;
    bool has_pg = false;
    size_t p = 0;
    while (p < text.size()) {
        size_t e = text.find('\n', p);
        if (e == std::string::npos) e = text.size();
        const std::string line = text.substr(p, e - p);
        p = e + 1;
        if (line.empty() || line[0] != '@') continue;
        const std::string tag = line.substr(1, 2);
        if (tag == "HD") {
            if (!HD.empty()) die("@HD tag can only present once!");
            HD = line + "\n";
        } else if (tag == "SQ") {
        } else if (tag == "RG") RG += line + "\n";
        else if (tag == "PG") {
            bool has_id = false;
            for (size_t q = 3; q < line.size();) {
                size_t t = line.find('\t', q + 1);
                if (t == std::string::npos) t = line.size();
                if (line.compare(q + 1, 3, "ID:") == 0) { has_id = true; if (line.substr(q + 4, t - q - 4) == "rsem-tbam2gbam") has_pg = true; }
                q = t;
            }
            if (!has_id) die("\"%s\" does not contain an ID!", line.c_str());
            PG += line + "\n";
        } else if (tag == "CO") CO += line + "\n";
        else other += line;  // (sic: the reference drops the newline of unknown records, SamHeader.cpp:108)
    }
    FILE* f = fopen(chrlist.c_str(), "r");
    if (!f) die("Cannot open %s! It may not exist.", chrlist.c_str());
    char* lb = nullptr;
    size_t cap = 0;
    ssize_t n;
    while ((n = getline(&lb, &cap, f)) >= 0) {
        std::string line(lb, (size_t)n);
        if (!line.empty() && line.back() == '\n') line.pop_back();
        const size_t pos = line.find('\t');
        if (pos == std::string::npos || pos == 0 || pos + 1 >= line.size() || line[pos + 1] == '\t') die("%s: a line without a name, a tab and a length", chrlist.c_str());
        // (sic: the count of the substring is the INDEX of the second tab, SamHeader.cpp:43 -- a third column comes along in part)
        SQ += "@SQ\tSN:" + line.substr(0, pos) + "\tLN:" + line.substr(pos + 1, line.find('\t', pos + 1)) + "\n";
    }
    free(lb);
    fclose(f);
    if (!has_pg) PG += "@PG\tID:rsem-tbam2gbam" + (command.empty() ? std::string() : "\tCL:" + command) + "\n";
    return HD + SQ + RG + PG + CO + other;
}

inline void convert_transcript_bam(const std::string& ref_name, const std::string& inF, const std::string& outF, const GbamOptions& opt, const std::string& command) {
    const auto t_all = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    const Transcripts T = load_transcripts(ref_name + ".ti");
    if (!opt.quiet) { printf("Start converting:\n"); fflush(stdout); }
    if (T.type != 0) die("Genome information is not provided! RSEM cannot convert the transcript bam file!");
    AlignmentReader in;
    in.open(inF);
    // Transcripts::buildMappings (Transcripts.h:105-143): the input's reference sequences are found by name
    const int n_targets = (int)in.header.names.size();
    if (n_targets <= 0) die("The SAM/BAM file declares less than one reference sequence!");
    if (n_targets > T.M) die("The SAM/BAM file declares more reference sequences (%d) than RSEM knows (%d)!", n_targets, T.M);
    if (n_targets < T.M)
        fprintf(stderr, "Warning: The SAM/BAM file declares less reference sequences (%d) than RSEM knows (%d)! Please make sure that you aligned your reads against transcript sequences instead of genome.\n", n_targets, T.M);
    std::vector<std::pair<std::string, int>> dict;
    for (int i = 1; i <= T.M; i++) dict.push_back({T.t[i].transcript_id, i});
    std::sort(dict.begin(), dict.end());
    for (size_t k = 1; k < dict.size(); k++)
        if (dict[k].first == dict[k - 1].first) die("RSEM's indices might be corrupted, %s appears more than once!", dict[k].first.c_str());
    std::vector<int32_t> e2t((size_t)n_targets);  // input tid -> transcript index of the handle (internal sid - 1)
    std::vector<char> seen((size_t)T.M + 1, 0);
    for (int k = 0; k < n_targets; k++) {
        auto it = std::lower_bound(dict.begin(), dict.end(), std::make_pair(in.header.names[k], -1));
        if (it == dict.end() || it->first != in.header.names[k]) die("RSEM can not recognize reference sequence name %s!", in.header.names[k].c_str());
        if (seen[it->second]) die("Reference sequence name %s appears more than once in the SAM/BAM file!", in.header.names[k].c_str());
        seen[it->second] = 1;
        e2t[k] = it->second - 1;
    }
    AlnHeader out_h;
    out_h.text = genome_header_text(in.header.text, ref_name + ".chrlist", command);
    parse_sq(out_h);
    // the handle: per transcript strand, length, the tid of its chromosome (refmap, BamConverter.h:63-66: the last of equal names), exons
    rsem_gmap* gm = nullptr;
    std::vector<uint8_t> strand((size_t)T.M);
    {
        std::vector<std::pair<std::string, int>> refmap;
        for (size_t i = 0; i < out_h.names.size(); i++) refmap.push_back({out_h.names[i], (int)i});
        std::stable_sort(refmap.begin(), refmap.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        std::vector<int32_t> length((size_t)T.M), out_tid((size_t)T.M), ex_s, ex_e;
        std::vector<uint64_t> ex_off(1, 0);
        for (int i = 1; i <= T.M; i++) {
            const TranscriptInfo& x = T.t[i];
            strand[i - 1] = (uint8_t)x.strand;
            length[i - 1] = x.length;
            auto it = std::upper_bound(refmap.begin(), refmap.end(), x.seqname, [](const std::string& v, const auto& a) { return v < a.first; });
            if (it == refmap.begin() || (it - 1)->first != x.seqname) die("%s.chrlist does not list %s, the sequence of transcript %s", ref_name.c_str(), x.seqname.c_str(), x.transcript_id.c_str());
            out_tid[i - 1] = (it - 1)->second;
            for (const auto& iv : x.structure) { ex_s.push_back(iv.first); ex_e.push_back(iv.second); }
            ex_off.push_back(ex_s.size());
        }
        const int rc = rsem_gmap_create(&gm, opt.device, T.M, strand.data(), length.data(), out_tid.data(), ex_off.data(), ex_s.data(), ex_e.data());
        if (rc != RSEM_OK) die("%s.ti: %s: %s", ref_name.c_str(), rsem_hip_strerror(rc), rsem_hip_last_error());
    }
    int nthreads = std::max(1, std::min(opt.threads, (int)std::max(1u, std::thread::hardware_concurrency())));
    if (const int granted = cgroup_cpu_cores()) nthreads = std::max(1, std::min(nthreads, granted));
    StagePool pool(nthreads);
    std::vector<BgzfDeflater> defl((size_t)nthreads);
    FILE* fo = fopen(outF.c_str(), "wb");
    if (!fo) die("Cannot open %s for writing!", outF.c_str());
    GbamStats S;
    {  // header
        std::vector<uint8_t> raw, comp;
        auto put = [&](const void* q, size_t n) { raw.insert(raw.end(), (const uint8_t*)q, (const uint8_t*)q + n); };
        put("BAM\1", 4);
        const int32_t l_text = (int32_t)out_h.text.size();
        put(&l_text, 4);
        put(out_h.text.data(), (size_t)l_text);
        const int32_t n_ref = (int32_t)out_h.names.size();
        put(&n_ref, 4);
        for (int i = 0; i < n_ref; i++) {
            const int32_t l_name = (int32_t)out_h.names[i].size() + 1;
            put(&l_name, 4);
            put(out_h.names[i].c_str(), (size_t)l_name);
            put(&out_h.lens[i], 4);
        }
        defl[0].stream(raw.data(), raw.size(), comp);
        if (fwrite(comp.data(), 1, comp.size(), fo) != comp.size()) die("Cannot write %s!", outF.c_str());
        S.out_bytes += comp.size();
    }
    size_t super_bytes = 64u << 20;
    if (const char* e = getenv("RSEM_HIP_BAM_CHUNK")) super_bytes = std::max<size_t>(64, (size_t)atoll(e));
    RecordChunks chunks(inF, in, pool, super_bytes);

    std::vector<RecView> fresh, recs;
    std::vector<std::vector<uint8_t>> held, held_next;  // the records of a group that the super-chunk's end may have cut
    int file_mates = 0;                                  // 1 or 2 once the first read is seen
    struct Unit { uint32_t rec; uint8_t mapped; };       // rec: its first record (read 1 of a pair is found when the fields are filled)
    struct Item { uint32_t group; uint32_t unit; };      // an output item: group (unit = ~0u) or an unmapped unit passed through
    std::vector<Unit> units;
    std::vector<Item> items;
    std::vector<uint64_t> group_off;
    std::vector<uint32_t> aln_unit;                      // alignment -> unit
    std::vector<int32_t> f_tr, f_pos, f_lq, o_tid, o_pos;
    std::vector<uint32_t> f_flag, o_flag, o_nc, o_bin, o_hasn, cigar;
    std::vector<uint64_t> coff, out_src, out_goff;
    std::vector<float> f_w, out_w;
    std::vector<uint8_t> first_is_2;                     // per alignment of a paired file: the records came read 2 first
    struct Piece { size_t b = 0, e = 0; std::vector<uint8_t> out; double asm_s = 0, defl_s = 0; };
    std::vector<Piece> pieces;
    bool last = false;
    auto t0 = std::chrono::steady_clock::now();
    while (chunks.next(fresh, last)) {
        recs.clear();
        for (const auto& h : held) recs.push_back({h.data(), h.size()});
        recs.insert(recs.end(), fresh.begin(), fresh.end());
        S.read_s += since(t0);
        t0 = std::chrono::steady_clock::now();
        // ---- cut: units, groups, output items (BamConverter::process, BamConverter.h:92-140)
        units.clear(); items.clear(); group_off.assign(1, 0); aln_unit.clear();
        size_t r = 0, n_keep = recs.size();
        std::pair<const char*, size_t> cq{nullptr, 0};
        bool open = false;           // a group is open
        size_t open_from = 0;        // its first record
        while (r < recs.size()) {
            if (recs[r].n < 32) die("%s: an alignment record of fewer than 32 bytes", inF.c_str());
            const uint32_t flag = (uint32_t)(recs[r].d[14] | (recs[r].d[15] << 8));
            const int mates = (flag & 1) ? 2 : 1;
            const auto name = canonical_name(recs[r]);
            if (file_mates == 0) file_mates = mates;
            if (mates != file_mates)
                die("Read %.*s: the file mixes single-end and paired-end reads, which the reference program does not define and this one does not support", (int)name.second, name.first);
            if (mates == 2 && r + 1 >= recs.size()) {
                if (!last) break;  // its mate is in the next super-chunk
                die("Read %.*s: the file ends before its second mate (the mates of a read must be adjacent)", (int)name.second, name.first);
            }
            const bool mapped = !(flag & 4);  // (of the record that comes first; a pair mapped on one side only stops the program below)
            const bool same = open && name.second == cq.second && !memcmp(name.first, cq.first, name.second);
            if (!mapped || !same) {
                if (open) group_off.push_back(aln_unit.size());
                open = false;
            }
            if (mapped) {
                if (!open) { open = true; open_from = r; cq = name; items.push_back({(uint32_t)(group_off.size() - 1), ~0u}); }
                aln_unit.push_back((uint32_t)units.size());
            } else items.push_back({0u, (uint32_t)units.size()});
            units.push_back({(uint32_t)r, (uint8_t)mapped});
            r += (size_t)mates;
        }
        if (!last && open) {  // the open group may go on: it waits, with whatever record follows it
            while (!aln_unit.empty() && units[aln_unit.back()].rec >= open_from) aln_unit.pop_back();
            while (!units.empty() && units.back().rec >= open_from) units.pop_back();
            items.pop_back();
            n_keep = open_from;
            open = false;
        } else {
            if (open) group_off.push_back(aln_unit.size());
            n_keep = r;
        }
        held_next.clear();
        for (size_t k = n_keep; k < recs.size(); k++) held_next.emplace_back(recs[k].d, recs[k].d + recs[k].n);
        const int mates = file_mates ? file_mates : 1;
        const size_t n_aln = aln_unit.size(), n_groups = group_off.size() - 1, n_mates = n_aln * (size_t)mates;
        S.cut_s += since(t0);
        t0 = std::chrono::steady_clock::now();
        // ---- fields, on the threads; the first record the program stops at is the one the reference stops at
        f_tr.resize(n_mates); f_pos.resize(n_mates); f_lq.resize(n_mates); f_flag.resize(n_mates); f_w.resize(n_aln); first_is_2.assign(n_aln, 0);
        const size_t n_units = units.size();
        const size_t npu = std::max<size_t>(1, std::min<size_t>((size_t)nthreads * 4, n_units / 256 + 1));
        std::vector<std::string> err(npu);
        std::vector<size_t> err_unit(npu, (size_t)-1);
        // (alignment index of a unit: units and alignments ascend together)
        std::vector<size_t> aln_of_piece(npu + 1, 0);
        {
            size_t a = 0;
            for (size_t i = 0; i <= npu; i++) {
                const size_t ub = n_units * i / npu;
                while (a < n_aln && aln_unit[a] < ub) a++;
                aln_of_piece[i] = a;
            }
        }
        pool.run(npu, [&](size_t i, int) {
            size_t a = aln_of_piece[i];
            for (size_t u = n_units * i / npu, ue = n_units * (i + 1) / npu; u < ue; u++) {
                const RecView *r1 = &recs[units[u].rec], *r2 = mates == 2 ? r1 + 1 : nullptr;
                auto stop = [&](const std::string& m) { err[i] = m; err_unit[i] = u; };
                RecCore c1, c2;
                if (!rec_core(*r1, c1) || (r2 && !rec_core(*r2, c2))) { stop("an alignment record is cut short"); return; }
                const auto name0 = canonical_name(*r1);
                bool swapped = false;
                if (r2) {
                    if (!(c2.flag & 1)) { stop("Read " + std::string(name0.first, name0.second) + ": its second record is not of a paired read (the mates of a read must be adjacent)"); return; }
                    if (!(c1.flag & 0x40)) { std::swap(r1, r2); std::swap(c1, c2); swapped = true; }
                    const auto nm = canonical_name(*r1);
                    if (!(c1.flag & 0x40) || !(c2.flag & 0x80)) { stop("Read " + std::string(nm.first, nm.second) + ": its two records are not read 1 and read 2"); return; }
                    if (!(c1.flag & 4) != !(c2.flag & 4)) {
                        stop("Detected partial alignments for read " + std::string(nm.first, nm.second) + ", which RSEM currently does not support!");
                        return;
                    }
                }
                if (!units[u].mapped) continue;
                const auto nm = canonical_name(*r1);
                if (r2 && c1.tid != c2.tid) { stop(std::string(nm.first, nm.second) + "'s two mates are aligned to two different transcripts!"); return; }
                if (c1.tid < 0 || c1.tid >= n_targets) { stop("Read " + std::string(nm.first, nm.second) + " is mapped but names no reference sequence of the header"); return; }
                if (c1.l_seq <= 0 || (r2 && c2.l_seq <= 0)) { stop("One alignment line has SEQ field as *. RSEM does not support this currently!"); return; }
                if (c1.pos < 0 || (r2 && c2.pos < 0)) { stop("Read " + std::string(nm.first, nm.second) + " is mapped but has no position"); return; }
                const size_t m0 = a * (size_t)mates;
                f_tr[m0] = e2t[c1.tid]; f_pos[m0] = c1.pos; f_lq[m0] = c1.l_seq; f_flag[m0] = c1.flag;
                if (r2) { f_tr[m0 + 1] = e2t[c2.tid]; f_pos[m0 + 1] = c2.pos; f_lq[m0 + 1] = c2.l_seq; f_flag[m0 + 1] = c2.flag; }
                f_w[a] = zw_weight(*r1, c1.aux_at);
                first_is_2[a] = swapped;
                a++;
            }
        });
        {
            size_t best = (size_t)-1, who = 0;
            for (size_t i = 0; i < npu; i++)
                if (err_unit[i] < best) { best = err_unit[i]; who = i; }
            if (best != (size_t)-1) die("%s", err[who].c_str());
        }
        S.fields_s += since(t0);
        t0 = std::chrono::steady_clock::now();
        // ---- device
        uint64_t cap = 0;
        for (size_t m = 0; m < n_mates; m++) cap += 2 * (uint64_t)T.t[f_tr[m] + 1].structure.size() + 2;
        o_tid.resize(n_mates); o_pos.resize(n_mates); o_flag.resize(n_mates); o_nc.resize(n_mates); o_bin.resize(n_mates); o_hasn.resize(n_mates);
        coff.resize(n_mates + 1); cigar.resize((size_t)cap + 1); out_src.resize(n_aln + 1); out_w.resize(n_aln + 1);
        rsem_gmap_info info;
        memset(&info, 0, sizeof(info));
        const int rc = rsem_gmap_convert(gm, mates, (int64_t)n_aln, (int64_t)n_groups, group_off.data(), f_tr.data(), f_pos.data(), f_lq.data(), f_flag.data(), f_w.data(),
                                         o_tid.data(), o_pos.data(), o_flag.data(), o_nc.data(), o_bin.data(), o_hasn.data(), coff.data(), cigar.data(), cap,
                                         out_src.data(), out_w.data(), &info);
        if (rc != RSEM_OK) die("%s: %s: %s (this program has no CPU path)", inF.c_str(), rsem_hip_strerror(rc), rsem_hip_last_error());
        const size_t n_out = (size_t)info.n_alignments_out;
        out_goff.assign(n_groups + 1, 0);  // where every group's output starts: the groups come out in their order
        {
            size_t k = 0;
            for (size_t g = 0; g < n_groups; g++) {
                out_goff[g] = k;
                while (k < n_out && out_src[k] < group_off[g + 1]) k++;
            }
            out_goff[n_groups] = k;
            if (k != n_out) die("internal error: %zu of %zu output alignments belong to a group", k, n_out);
        }
        S.device_s += since(t0);
        S.calls++; S.batches += (uint64_t)info.n_batches; S.upload_ms += info.upload_ms; S.kernel_ms += info.kernel_ms;
        S.groups += n_groups; S.aln_in += n_aln; S.aln_out += n_out; S.cigar_words += info.n_cigar_words; S.records += n_keep;
        t0 = std::chrono::steady_clock::now();
        // ---- assemble and deflate: the items in pieces, on the threads
        const size_t n_items = items.size();
        const size_t np = std::max<size_t>(1, std::min<size_t>((size_t)nthreads * 4, n_items / 64 + 1));
        pieces.assign(np, Piece());
        for (size_t i = 0; i < np; i++) { pieces[i].b = n_items * i / np; pieces[i].e = n_items * (i + 1) / np; }
        pool.run(np, [&](size_t i, int me) {
            Piece& P = pieces[i];
            const auto ta = std::chrono::steady_clock::now();
            std::vector<uint8_t> raw;
            auto copy_through = [&](const RecView& rv) {
                const int32_t bs = (int32_t)rv.n;
                raw.insert(raw.end(), (const uint8_t*)&bs, (const uint8_t*)&bs + 4);
                raw.insert(raw.end(), rv.d, rv.d + rv.n);
            };
            for (size_t it = P.b; it < P.e; it++) {
                if (items[it].unit != ~0u) {  // an unmapped read: both records as they are, in their order
                    const uint32_t r0 = units[items[it].unit].rec;
                    const bool swap = mates == 2 && !(recs[r0].d[14] & 0x40);
                    copy_through(recs[r0 + (swap ? 1 : 0)]);
                    if (mates == 2) copy_through(recs[r0 + (swap ? 0 : 1)]);
                    continue;
                }
                const uint32_t g = items[it].group;
                for (size_t k = out_goff[g]; k < out_goff[g + 1]; k++) {
                    const size_t a = (size_t)out_src[k];
                    const uint32_t r0 = units[aln_unit[a]].rec;
                    const float w = out_w[k];
                    size_t zw1 = 0, rec1 = 0;
                    for (int m = 0; m < mates; m++) {
                        const size_t mi = a * (size_t)mates + (size_t)m;
                        const RecView& rv = recs[r0 + (size_t)(first_is_2[a] ? 1 - m : m)];
                        RecCore c;
                        rec_core(rv, c);
                        MateOut mo;
                        mo.tid = o_tid[mi]; mo.pos = o_pos[mi]; mo.flag = o_flag[mi]; mo.n_cigar = o_nc[mi]; mo.bin = o_bin[mi]; mo.has_n = o_hasn[mi];
                        mo.cigar = cigar.data() + coff[mi];
                        mo.minus = strand[(size_t)f_tr[mi]] == '-';
                        mo.paired = (c.flag & 1) != 0;
                        mo.mate_pos = mates == 2 ? o_pos[a * 2 + (size_t)(1 - m)] : 0;
                        size_t zw = 0;
                        const size_t at = assemble_record(raw, rv, c, mo, zw);
                        if (m == 0) {
                            zw1 = zw; rec1 = at;
                            if (zw) { put_weight(raw, zw, w); raw[at + 4 + 9] = prb_to_mapq(w); }  // (float -> double, as the reference's call)
                        } else {
                            if (zw1 && zw) put_weight(raw, zw, w);
                            raw[at + 4 + 9] = raw[rec1 + 4 + 9];
                        }
                    }
                }
            }
            P.asm_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - ta).count();
            const auto td = std::chrono::steady_clock::now();
            defl[me].stream(raw.data(), raw.size(), P.out);
            P.defl_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - td).count();
        });
        {
            // (the stage's wall clock, split by where the threads' time went)
            double a = 0, d = 0;
            for (const Piece& P : pieces) { a += P.asm_s; d += P.defl_s; }
            const double wall = since(t0);
            if (a + d > 0) { S.assemble_s += wall * a / (a + d); S.deflate_s += wall * d / (a + d); }
        }
        t0 = std::chrono::steady_clock::now();
        for (Piece& P : pieces) {
            if (!P.out.empty() && fwrite(P.out.data(), 1, P.out.size(), fo) != P.out.size()) die("Cannot write %s!", outF.c_str());
            S.out_bytes += P.out.size();
        }
        S.write_s += since(t0);
        if (!opt.quiet) {  // BamConverter.h:104: a dot per million records
            static uint64_t dots = 0;
            for (; (dots + 1) * 1000000 <= S.records; dots++) { printf("."); fflush(stdout); }
        }
        held.swap(held_next);
        t0 = std::chrono::steady_clock::now();
    }
    rsem_gmap_destroy(gm);
    bgzf_write_eof(fo);
    if (fclose(fo) != 0) die("Cannot write %s!", outF.c_str());
    if (!opt.quiet) {
        if (S.records >= 1000000) printf("\n");
        printf("Genome bam file is generated!\n");
    }
    if (getenv("RSEM_HIP_TIMING"))
        printf("[timing] {\"wall_s\": %.4f, \"inflate_cut_s\": %.4f, \"fields_s\": %.4f, \"device_call_s\": %.4f, \"upload_ms\": %.3f, \"kernel_ms\": %.3f, "
               "\"assemble_s\": %.4f, \"deflate_s\": %.4f, \"write_s\": %.4f, \"threads\": %d, \"records\": %llu, \"groups\": %llu, \"alignments_in\": %llu, "
               "\"alignments_out\": %llu, \"cigar_words\": %llu, \"device_calls\": %llu, \"batches\": %llu, \"out_bytes\": %llu}\n",
               since(t_all), S.read_s + S.cut_s, S.fields_s, S.device_s, S.upload_ms, S.kernel_ms, S.assemble_s, S.deflate_s, S.write_s, nthreads,
               (unsigned long long)S.records, (unsigned long long)S.groups, (unsigned long long)S.aln_in, (unsigned long long)S.aln_out,
               (unsigned long long)S.cigar_words, (unsigned long long)S.calls, (unsigned long long)S.batches, (unsigned long long)S.out_bytes);
}

}  // namespace rsemh
