// refprep_host.hpp -- host side of rsem-extract-reference-transcripts, rsem-synthesis-reference-transcripts and rsem-preref
// (DESIGN.md section 13): FASTA framing, the GTF, the mapping files, .ti / .grp / .chrlist / .seq text and the order in which the
// reference's errors come.  Every sequence byte of the outputs comes off the device (rsem_refseq_load / rsem_refseq_gather,
// rsem_amd/csrc/refseq.hip); name lines, numbers and mask words are written here.  Each function cites the reference code it restates.
#pragma once
#include <time.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../../include/rsem_hip.h"
#include "files.hpp"

namespace rsemh {

constexpr int kMaxWarns = 50;  // utils.h:26

inline bool c_isspace(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// the first whitespace-delimited token of [p, e), as `istringstream >> s` takes it; false (s untouched) where there is none
inline bool first_token(const char* p, const char* e, std::string& s, const char** rest = nullptr) {
    while (p < e && c_isspace(*p)) p++;
    if (p == e) { if (rest) *rest = e; return false; }
    const char* q = p;
    while (q < e && !c_isspace(*q)) q++;
    s.assign(p, q);
    if (rest) *rest = q;
    return true;
}

// ---- the device -------------------------------------------------------------------------------------------------------------

inline void refseq_try(int rc, const char* what) {
    if (rc != RSEM_OK) die("%s: %s: %s", what, rsem_hip_strerror(rc), rsem_hip_last_error());
}

// `--device d` as the last two arguments of a program whose argv ends in a file list
inline int strip_device(int& argc, char* argv[]) {
    if (argc >= 3 && !strcmp(argv[argc - 2], "--device")) {
        const int d = atoi(argv[argc - 1]);
        argc -= 2;
        return d;
    }
    return 0;
}

// Where the time goes, for tools/time_refprep.py: with RSEM_REFPREP_STAGES=<file> in the environment a program leaves one JSON object
// there -- its wall clock by stage and the handle's counters (bytes by construction, HIP-event times).  Nothing else depends on it.
inline double now_ms() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
struct Stages {
    double t_start = now_ms(), device_ms = 0, write_ms = 0, mark = 0;
    void device_begin() { mark = now_ms(); }
    void device_end() { device_ms += now_ms() - mark; }
    void write_begin() { mark = now_ms(); }
    void write_end() { write_ms += now_ms() - mark; }
    void report(const char* program, rsem_refseq* h) const {
        const char* path = getenv("RSEM_REFPREP_STAGES");
        if (!path || !*path) return;
        rsem_refseq_info I;
        memset(&I, 0, sizeof(I));
        if (h) (void)rsem_refseq_get_info(h, &I);
        FILE* f = fopen(path, "w");
        if (!f) return;
        const double total = now_ms() - t_start;
        fprintf(f, "{\"program\": \"%s\", \"total_ms\": %.3f, \"read_and_frame_ms\": %.3f, \"device_calls_ms\": %.3f, \"write_ms\": %.3f, "
                   "\"upload_ms\": %.3f, \"kernel_ms\": %.3f, \"download_ms\": %.3f, \"n_records\": %llu, \"raw_bytes\": %llu, \"n_bases\": %llu, "
                   "\"n_segments\": %llu, \"gathered_bytes\": %llu, \"n_batches\": %d, \"n_launches\": %d, \"batch_bytes\": %llu, \"device_bytes\": %llu}\n",
                program, total, total - device_ms - write_ms, device_ms, write_ms, I.upload_ms, I.kernel_ms, I.download_ms, (unsigned long long)I.n_records,
                (unsigned long long)I.raw_bytes, (unsigned long long)I.n_bases, (unsigned long long)I.n_segments, (unsigned long long)I.gathered_bytes, I.n_batches,
                I.n_launches, (unsigned long long)I.batch_bytes, (unsigned long long)I.device_bytes);
        fclose(f);
    }
};

// ---- FASTA framing (extractRef.cpp:336-349, synthesisRef.cpp:175-188, Refs.h:96-102) -----------------------------------------

struct FastaRecord {
    uint64_t head_lo, head_hi;  // the header line behind '>' , without its line end
    uint64_t lo, hi;            // the body: every line up to the next line that starts with '>'
};

// Nothing where the file is empty or its first line does not start with '>' (getline, then `while (fin && line[0] == '>')`).
inline std::vector<FastaRecord> frame_fasta(const char* d, size_t n) {
    std::vector<FastaRecord> recs;
    if (n == 0 || d[0] != '>') return recs;
    size_t h = 0;
    while (h < n) {
        FastaRecord r;
        r.head_lo = h + 1;
        const char* nl = (const char*)memchr(d + h, '\n', n - h);
        r.head_hi = nl ? (size_t)(nl - d) : n;
        r.lo = nl ? r.head_hi + 1 : n;
        size_t q = r.lo;  // the next '>' at a line's start
        for (;;) {
            const char* g = q < n ? (const char*)memchr(d + q, '>', n - q) : nullptr;
            if (!g) { q = n; break; }
            q = (size_t)(g - d);
            if (q == r.lo || d[q - 1] == '\n') break;
            q++;
        }
        r.hi = q;
        recs.push_back(r);
        h = q;
    }
    return recs;
}

// check()'s message for the byte at `off` (extractRef.cpp:297-299): the line and position getline's loop had reached
[[noreturn]] inline void die_bad_character(const char* file, const char* d, uint64_t off) {
    int line = 1;
    uint64_t start = 0;
    for (const char* p = d; (p = (const char*)memchr(p, '\n', (size_t)(d + off - p))) != nullptr; p++) { line++; start = (uint64_t)(p - d) + 1; }
    const char c = d[off];
    fprintf(stderr, "FASTA file %s contains an unknown character, %c (ASCII code %d), at line %d, position %d!\n", file, c, (int)(signed char)c, line,
            (int)(off - start) + 1);
    exit(-1);
}

// the records of one file through the device, a batch at a time; after each batch `visit(r, n_bases, bad)` sees its records in order
// (it stops the program at the first error) and `after_batch(first, last)` may gather from the records while they are resident
template <class Visit, class After>
inline void load_file(rsem_refseq* h, int mode, const char* d, const std::vector<FastaRecord>& recs, const std::vector<uint8_t>* keep, Visit visit, After after_batch) {
    const int64_t n = (int64_t)recs.size();
    if (!n) return;
    std::vector<uint64_t> lo((size_t)n), hi((size_t)n), nb((size_t)n);
    std::vector<int64_t> bad((size_t)n);
    for (int64_t r = 0; r < n; r++) { lo[r] = recs[r].lo; hi[r] = recs[r].hi; }
    for (int64_t first = 0; first < n;) {
        int64_t taken = 0;
        refseq_try(rsem_refseq_load(h, mode, (const uint8_t*)d, n, lo.data(), hi.data(), keep ? keep->data() : nullptr, first, &taken, nb.data(), bad.data()),
                   "rsem_refseq_load");
        for (int64_t r = first; r < first + taken; r++) visit(r, nb[r], bad[r]);
        after_batch(first, first + taken);
        first += taken;
    }
}

// ---- the GTF (GTFItem.h, extractRef.cpp:89-216) ------------------------------------------------------------------------------

struct Interval { int start, end; };

struct RefTranscript {  // Transcript.h
    std::string transcript_id, gene_id, seqname, gene_name, transcript_name, left;
    char strand = '+';
    int length = 0;
    std::vector<Interval> structure;
};

[[noreturn]] inline void gtf_die(const std::string& line, const std::string& msg) {  // GTFItem.h:174-181
    fprintf(stderr, "The GTF file might be corrupted!\n");
    fprintf(stderr, "Stop at line : %s\n", line.c_str());
    fprintf(stderr, "Error Message: %s\n", msg.c_str());
    exit(-1);
}

struct GtfItem {
    std::string seqname, source, feature, score, frame, gene_id, transcript_id, gene_name, transcript_name, left;
    int start = 0, end = 0;
    char strand = 0;

    // GTFItem::parse: nine getlines on one istringstream -- once the line's end is reached a later field KEEPS what it held (the item
    // is reused from line to line; the local tmp starts empty)
    void parse(const std::string& line) {
        size_t cur = 0;
        bool eof = false;
        auto get = [&](std::string& f, char delim) {
            if (eof) return;
            const size_t p = delim ? line.find(delim, cur) : std::string::npos;
            if (p == std::string::npos) { f.assign(line, cur, std::string::npos); eof = true; }
            else { f.assign(line, cur, p - cur); cur = p + 1; }
        };
        std::string tmp;
        get(seqname, '\t'); get(source, '\t'); get(feature, '\t');
        get(tmp, '\t'); start = atoi(tmp.c_str());
        get(tmp, '\t'); end = atoi(tmp.c_str());
        get(score, '\t');
        get(tmp, '\t');
        if (!(tmp.length() == 1 && (tmp[0] == '+' || tmp[0] == '-'))) gtf_die(line, "Strand is neither '+' nor '-'!");
        strand = tmp[0];
        get(frame, '\t');
        get(left, 0);
    }

    bool get_an_attribute(int& lpos, int& rpos, int left_len) const {  // GTFItem.h:160-172
        while (lpos < left_len && c_isspace(left[lpos])) ++lpos;
        rpos = lpos;
        bool in_quote = false;
        while (rpos < left_len && (left[rpos] != ';' || in_quote)) {
            if (left[rpos] == '"') in_quote ^= true;
            ++rpos;
        }
        return rpos < left_len;
    }

    void parse_attributes(const std::string& line) {  // GTFItem.h:71-123
        gene_id = transcript_id = gene_name = transcript_name = "";
        int nleft = 4, pos, lpos = 0, rpos, left_len = (int)left.length();
        std::string identifier;
        auto at = [&](int i) { return i >= 0 && i < left_len ? left[i] : '\0'; };
        while (nleft > 0 && get_an_attribute(lpos, rpos, left_len)) {
            pos = lpos;
            while (pos < rpos && !c_isspace(at(pos))) ++pos;
            if (!c_isspace(at(pos))) gtf_die(line, "Cannot locate the identifier from attribute " + left.substr(lpos, rpos + 1 - lpos) + "!");
            identifier = left.substr(lpos, pos - lpos);
            lpos = rpos + 1;
            ++pos;
            while (pos < rpos && c_isspace(at(pos))) ++pos;
            if (at(pos) != '"') pos = rpos;
            --rpos;
            while (rpos > pos && c_isspace(at(rpos))) --rpos;
            if (rpos > pos && at(rpos) != '"') rpos = pos;
            const char* empty = "'s value should be surrounded by double quotes and cannot be empty!";
            if (identifier == "gene_id") {
                if (gene_id != "") gtf_die(line, "gene_id appear more than once!");
                if (!(rpos - pos > 1)) gtf_die(line, "Attribute " + identifier + empty);
                gene_id = left.substr(pos + 1, rpos - pos - 1);
                --nleft;
            } else if (identifier == "transcript_id") {
                if (transcript_id != "") gtf_die(line, "transcript_id appear more than once!");
                if (!(rpos - pos > 1)) gtf_die(line, "Attribute " + identifier + empty);
                transcript_id = left.substr(pos + 1, rpos - pos - 1);
                --nleft;
            } else if (identifier == "gene_name" && gene_name == "" && rpos - pos > 1) {
                gene_name = left.substr(pos + 1, rpos - pos - 1);
                --nleft;
            } else if (identifier == "transcript_name" && transcript_name == "" && rpos - pos > 1) {
                transcript_name = left.substr(pos + 1, rpos - pos - 1);
                --nleft;
            }
        }
        if (gene_id == "") gtf_die(line, "Cannot find gene_id!");
        if (transcript_id == "") gtf_die(line, "Cannot find transcript_id!");
    }
};

// cleanStr (utils.h:117-127)
inline std::string clean_str(const std::string& s) {
    int len = (int)s.length(), fr = 0, to = len - 1;
    while (fr < len && c_isspace(s[fr])) ++fr;
    while (to >= 0 && c_isspace(s[to])) --to;
    return fr <= to ? s.substr(fr, to - fr + 1) : "";
}

template <class Fn>
inline void for_each_line(const MappedFile& f, Fn fn) {  // getline: the last line need not end in '\n'
    std::string line;
    for (size_t p = 0; p < f.size;) {
        const char* nl = (const char*)memchr(f.data + p, '\n', f.size - p);
        const size_t e = nl ? (size_t)(nl - f.data) : f.size;
        line.assign(f.data + p, e - p);
        fn(line);
        p = e + 1;
    }
}

// loadMappingInfo (extractRef.cpp:71-87; synthesisRef.cpp:37-70 with file_type 2): `strin >> value [>> value2] >> key` into strings
// that live across the lines, so a line with fewer tokens keeps the earlier ones
inline void load_mapping_info(int file_type, const char* path, std::map<std::string, std::string>& t1, std::map<std::string, std::string>& t2) {
    MappedFile f;
    if (!f.open(path)) die("Cannot open %s! It may not exist.", path);
    std::string key, value, value2;
    for_each_line(f, [&](const std::string& raw_line) {
        const std::string line = clean_str(raw_line);
        if (!line.empty() && line[0] == '#') return;
        const char *p = line.data(), *e = p + line.size();
        if (first_token(p, e, value, &p) && (file_type != 2 || first_token(p, e, value2, &p))) first_token(p, e, key, &p);
        t1[key] = value;
        if (file_type == 2) t2[key] = value2;
    });
}

struct GtfResult {
    std::vector<RefTranscript> tr;                   // 1-based: tr[0] is not used
    std::map<std::string, std::vector<int>> sn2tr;  // chromosome -> its transcripts, ascending
};

inline void general_die(const std::string& msg) { fprintf(stderr, "%s\n", msg.c_str()); exit(-1); }  // my_assert.h:37-41

// Transcript's constructor (Transcript.h:38-51): leading spaces -- not tabs -- leave `left`
inline std::string strip_left(const std::string& left) {
    size_t pos = 0;
    while (pos < left.length() && left[pos] == ' ') ++pos;
    return left.substr(pos);
}

// parse_gtf_file + buildTranscript (extractRef.cpp:89-216); the sort is stable, where the reference's leaves equal keys open
inline GtfResult parse_gtf(const char* path, const std::set<std::string>& sources, bool has_mapping, const std::map<std::string, std::string>& mi_table, bool verbose) {
    MappedFile f;
    if (!f.open(path)) die("Cannot open %s! It may not exist.", path);
    std::vector<GtfItem> items;
    GtfItem item;
    int cnt = 0, n_warns = 0;
    for_each_line(f, [&](const std::string& line) {
        if (!line.empty() && line[0] == '#') return;
        item.parse(line);
        if (item.feature == "exon" && (sources.empty() || sources.count(item.source))) {
            if (item.start > item.end) {
                if (++n_warns <= kMaxWarns) {
                    fprintf(stderr, "Warning: exon's start position is larger than its end position! This exon is discarded.\n");
                    fprintf(stderr, "\t%s\n\n", line.c_str());
                }
            } else if (item.start < 1) {
                if (++n_warns <= kMaxWarns) {
                    fprintf(stderr, "Warning: exon's start position is less than 1! This exon is discarded.\n");
                    fprintf(stderr, "\t%s\n\n", line.c_str());
                }
            } else {
                item.parse_attributes(line);
                if (has_mapping) {
                    auto it = mi_table.find(item.transcript_id);
                    if (it == mi_table.end()) general_die("Mapping Info is not correct, cannot find " + item.transcript_id + "'s gene_id!");
                    item.gene_id = it->second;
                }
                items.push_back(item);
            }
        }
        ++cnt;
        if (verbose && cnt % 200000 == 0) printf("Parsed %d lines\n", cnt);
    });
    if (n_warns > 0) fprintf(stderr, "Warning: In total, %d exons are discarded.", n_warns);
    std::stable_sort(items.begin(), items.end(), [](const GtfItem& a, const GtfItem& b) {
        if (a.gene_id != b.gene_id) return a.gene_id < b.gene_id;
        if (a.transcript_id != b.transcript_id) return a.transcript_id < b.transcript_id;
        return a.start < b.start;
    });
    GtfResult G;
    G.tr.emplace_back();
    const int n_items = (int)items.size();
    for (int sp = 0; sp < n_items;) {
        int ep = sp + 1;
        while (ep < n_items && items[ep].transcript_id == items[sp].transcript_id) ep++;
        RefTranscript t;
        t.transcript_id = items[sp].transcript_id;
        t.gene_id = items[sp].gene_id;
        t.strand = items[sp].strand;
        t.seqname = items[sp].seqname;
        t.left = strip_left(items[sp].left);
        int cur_s = -1, cur_e = -1;
        for (int i = sp; i < ep; i++) {
            const GtfItem& it = items[i];
            if (t.strand != it.strand) general_die("According to the GTF file given, transcript " + t.transcript_id + " has exons from different orientations!");
            if (t.seqname != it.seqname) general_die("According to the GTF file given, transcript " + t.transcript_id + " has exons on multiple chromosomes!");
            if (it.gene_name != "") {
                if (t.gene_name == "") t.gene_name = it.gene_name;
                else if (t.gene_name != it.gene_name) general_die("Transcript " + t.transcript_id + " is associated with multiple gene names!");
            }
            if (it.transcript_name != "") {
                if (t.transcript_name == "") t.transcript_name = it.transcript_name;
                else if (t.transcript_name != it.transcript_name) general_die("Transcript " + t.transcript_id + " is associated with multiple transcript names!");
            }
            if ((long long)cur_e + 1 < it.start) {
                if (cur_s > 0) t.structure.push_back({cur_s, cur_e});
                cur_s = it.start;
            }
            cur_e = cur_e < it.end ? it.end : cur_e;
        }
        if (cur_s > 0) t.structure.push_back({cur_s, cur_e});
        for (const Interval& iv : t.structure) t.length += iv.end + 1 - iv.start;
        G.sn2tr[t.seqname].push_back((int)G.tr.size());
        G.tr.push_back(std::move(t));
        sp = ep;
    }
    if (G.tr.size() <= 1) general_die("The reference contains no transcripts!");
    if (verbose) printf("Parsing gtf File is done!\n");
    return G;
}

// ---- writers ------------------------------------------------------------------------------------------------------------------

struct OutFile {  // a buffered file that stops the program when it cannot be written
    FILE* f = nullptr;
    std::string path;
    explicit OutFile(const std::string& p) : path(p) {
        f = fopen(p.c_str(), "w");
        if (f) setvbuf(f, nullptr, _IOFBF, 1 << 20);
    }
    void put(const void* p, size_t n) { if (f && n) fwrite(p, 1, n, f); }
    void put(const std::string& s) { put(s.data(), s.size()); }
    void close() { if (f) { fclose(f); f = nullptr; } }
    ~OutFile() { close(); }
};

// Transcripts::writeTo, Transcript::write (Transcripts.h:96-103, Transcript.h:150-167); tr is 1-based, ids[k] the k-th to write
inline void write_ti(const std::string& path, const std::vector<RefTranscript>& tr, const std::vector<int>& ids, int type) {
    OutFile o(path);
    o.put(std::to_string(ids.size()) + " " + std::to_string(type) + "\n");
    std::string s;
    for (int id : ids) {
        const RefTranscript& t = tr[id];
        s = t.transcript_id;
        if (t.transcript_name != "") s += "\t" + t.transcript_name;
        s += "\n" + t.gene_id;
        if (t.gene_name != "") s += "\t" + t.gene_name;
        s += "\n" + t.seqname + "\n" + std::string(1, t.strand) + " " + std::to_string(t.length) + "\n" + std::to_string(t.structure.size());
        for (const Interval& iv : t.structure) s += " " + std::to_string(iv.start) + " " + std::to_string(iv.end);
        s += "\n" + t.left + "\n";
        o.put(s);
    }
}

inline void write_numbers(const std::string& path, const std::vector<int>& v) {
    OutFile o(path);
    for (int x : v) o.put(std::to_string(x) + "\n");
}

}  // namespace rsemh
