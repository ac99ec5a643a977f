// fasta_codes.hpp -- the FASTA reader of rsem-for-ebseq-calculate-clustering-info: the reference's loadRef + convert
// (EBSeq/calcClusteringInfo.cpp:51-90), straight into base codes.
//
// The rules are the reference's getline loop's:
//   - the file is taken line by line at '\n'; a '\r' in front of it stays in the line (it is part of a header, and a base like any
//     other byte of a sequence line);
//   - an entry is a line that starts with '>' (its name: everything behind the '>') and the lines up to the next such line, joined;
//   - reading stops at the first line in entry position that does not start with '>' (so a file that starts otherwise has no entry);
//   - an entry whose lines are all empty is dropped with a warning on stdout;
//   - letters are upper-cased; A C G T are the codes 0 1 2 3 and EVERY other byte is N, code 4.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "files.hpp"

namespace rsemh {

struct FastaCodes {
    std::vector<std::string> names;
    std::vector<uint64_t> seq_off{0};  // entry t = codes[seq_off[t] .. seq_off[t+1])
    std::vector<uint8_t> codes;
    int M() const { return (int)names.size(); }
};

inline const uint8_t* base_code_table() {
    static uint8_t table[256];
    static bool made = false;
    if (!made) {
        for (int i = 0; i < 256; i++) table[i] = 4;
        table['A'] = table['a'] = 0;
        table['C'] = table['c'] = 1;
        table['G'] = table['g'] = 2;
        table['T'] = table['t'] = 3;
        made = true;
    }
    return table;
}

// false: the file cannot be opened
inline bool read_fasta_codes(const std::string& path, FastaCodes& out) {
    MappedFile f;
    if (!f.open(path)) return false;
    const uint8_t* code = base_code_table();
    const char* p = f.data;
    const char* const end = f.data + f.size;
    // one line: [b, e), without its '\n'; false at the end of the file (a last line without '\n' is a line)
    auto next_line = [&](const char*& b, const char*& e) {
        if (p >= end) return false;
        b = p;
        const char* nl = (const char*)memchr(p, '\n', (size_t)(end - p));
        e = nl ? nl : end;
        p = nl ? nl + 1 : end;
        return true;
    };
    out.codes.reserve(f.size);
    const char *b, *e;
    bool have = next_line(b, e);
    while (have && e > b && *b == '>') {
        const std::string tag(b + 1, e);
        const size_t start = out.codes.size();
        while ((have = next_line(b, e)) && !(e > b && *b == '>'))
            for (const char* c = b; c < e; c++) out.codes.push_back(code[(unsigned char)*c]);
        if (out.codes.size() == start) {
            printf("Warning: Fasta entry %s has an empty sequence! It is omitted!\n", tag.c_str());
            continue;
        }
        out.names.push_back(tag);
        out.seq_off.push_back(out.codes.size());
    }
    return true;
}

}  // namespace rsemh
