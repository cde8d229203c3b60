// hammock_targets.hpp -- the targets FASTA of `hammock-hip scan`: long sequences (an antigen, a proteome) as hmk_set_targets takes
// them.  Not Hammock's peptide loader: a sequence may span lines, the name is the header up to the first white space, records are
// never merged (two equal proteins stay two targets), and a record has HMK_MAX_LEN + 1 .. HMK_TARGET_MAX_LEN residues of the same
// 24 letters (UniqueSequence.java:23-26).  Standard C++ only: tests/tools/scan_host_check.cpp runs it under the sanitizers.
#ifndef HAMMOCK_TARGETS_HPP
#define HAMMOCK_TARGETS_HPP

#include <cctype>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace hammock {

struct TargetFormatError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

struct TargetSet {
    std::vector<std::string> names;
    std::vector<uint8_t> residues;          // codes 0..23, concatenated
    std::vector<uint64_t> offsets{0};       // names.size() + 1
    size_t size() const { return names.size(); }
    uint64_t length(size_t t) const { return offsets[t + 1] - offsets[t]; }
};

inline TargetSet loadTargetsFromFasta(const std::string &fileName, uint64_t minLength, uint64_t maxLength) {
    static const char LETTERS[25] = "ARNDCQEGHILKMFPSTWYVBZX*";
    std::ifstream in(fileName);
    if (!in) throw TargetFormatError("Error. Cannot read the targets file " + fileName);
    TargetSet set;
    bool open = false;
    auto describe = [&]() { return "record " + std::to_string(set.names.size()) + " (\"" + set.names.back() + "\") of " + fileName; };
    auto close = [&]() {
        if (!open) return;
        const uint64_t n = set.residues.size() - set.offsets.back();
        if (n < minLength)
            throw TargetFormatError("Error. Target " + describe() + " has " + std::to_string(n) + " residues: a target has at least " +
                                    std::to_string(minLength) + ". Shorter sequences are peptides: score them with mode search.");
        if (n > maxLength)
            throw TargetFormatError("Error. Target " + describe() + " has " + std::to_string(n) + " residues: at most " + std::to_string(maxLength) +
                                    " are taken. Cut it into overlapping pieces.");
        set.offsets.push_back(set.residues.size());
    };
    std::string line;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '>') {
            close();
            size_t e = 1;
            while (e < line.size() && !std::isspace((unsigned char)line[e])) e++;
            set.names.push_back(line.substr(1, e - 1));
            open = true;
            continue;
        }
        for (char ch : line) {
            if (std::isspace((unsigned char)ch)) continue;
            if (!open) throw TargetFormatError("Error. The targets file " + fileName + " does not start with a '>' header line.");
            const char up = (char)std::toupper((unsigned char)ch);
            const char *f = up ? std::strchr(LETTERS, up) : nullptr;
            if (!f) throw TargetFormatError("Error. Target " + describe() + " contains '" + std::string(1, ch) + "', which is not an amino acid letter.");
            set.residues.push_back((uint8_t)(f - LETTERS));
        }
    }
    close();
    return set;
}

}  // namespace hammock
#endif
