// The vw namespace map and the VW text parser's state (parser.cpp), shared with the device text route (text_parser.cpp), which
// uploads the same name table and hands the lines it does not take to the same parser.  Not part of the C ABI.
#pragma once

#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "fwgpu_internal.h"

namespace fwgpu {

struct VwEntry {
    std::string vwname, verbose;
    uint32_t index;
    bool f32;
};

}  // namespace fwgpu

struct fwgpu_vwmap {
    std::vector<fwgpu::VwEntry> entries;  // vw_source.entries
    uint32_t skip_prefix = 0;             // vw_source.namespace_skip_prefix
    uint32_t num_namespaces = 0;          // max index + 1 (vwmap.rs:83-88)
    std::unordered_map<std::string, uint32_t> by_vwname, by_verbose;  // -> entries index

    void finish() {  // vwmap.rs:54-89 new_from_source
        num_namespaces = 0;
        by_vwname.clear();
        by_verbose.clear();
        for (uint32_t i = 0; i < entries.size(); i++) {
            by_vwname[entries[i].vwname] = i;
            by_verbose[entries[i].verbose] = i;
            num_namespaces = std::max(num_namespaces, entries[i].index);
        }
        num_namespaces += 1;
    }
};

struct fwgpu_parser {
    const fwgpu_vwmap *vw;  // copied
    fwgpu_vwmap vw_copy;
    std::vector<uint32_t> seed;  // murmur3::hash32(vwname) per entry (parser.rs:83)
    std::vector<uint32_t> out;   // output_buffer
    std::string scratch;         // padded copy of a line that has no readable byte after it
    std::vector<uint32_t> delta; // candidate-only form of the last record (fwgpu_parser_parse_candidate)
    std::string cmd_arg;         // filename of the last hogwild_load command
    // vwname -> entry: the reference walks a 256-ary radix tree (radix_tree.rs); a small open-addressing table on the
    // name's bytes does the same exact-match lookup without allocating
    std::vector<int32_t> ns_table;
    uint32_t ns_mask = 0;
    static uint32_t name_hash(const unsigned char *s, size_t n) {
        uint32_t h = 2166136261u;
        for (size_t i = 0; i < n; i++) h = (h ^ s[i]) * 16777619u;
        return h;
    }
    void build_ns_table() {
        uint32_t cap = 16;
        while (cap < 4 * vw_copy.entries.size()) cap <<= 1;
        ns_table.assign(cap, -1);
        ns_mask = cap - 1;
        for (size_t i = 0; i < vw_copy.entries.size(); i++) {
            const std::string &nm = vw_copy.entries[i].vwname;
            // later entries with the same vwname replace earlier ones, like HashMap::insert (vwmap.rs:75-78)
            uint32_t slot = name_hash(reinterpret_cast<const unsigned char *>(nm.data()), nm.size()) & ns_mask;
            while (ns_table[slot] >= 0 && vw_copy.entries[ns_table[slot]].vwname != nm) slot = (slot + 1) & ns_mask;
            ns_table[slot] = (int32_t)i;
        }
    }
    int find_ns(const unsigned char *s, size_t n) const {
        uint32_t slot = name_hash(s, n) & ns_mask;
        while (ns_table[slot] >= 0) {
            const std::string &nm = vw_copy.entries[ns_table[slot]].vwname;
            if (nm.size() == n && std::memcmp(nm.data(), s, n) == 0) return ns_table[slot];
            slot = (slot + 1) & ns_mask;
        }
        return -1;
    }
};
