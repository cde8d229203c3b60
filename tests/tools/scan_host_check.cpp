// scan_host_check.cpp -- a stand-alone program over the host-only code of the scan for a sanitizer build on the CPU:
// the targets loader (hammock_amd/host/hammock_targets.hpp) and the planner's class rule (hammock_amd/csrc/hmk_scan.h).  No GPU, no
// library, nothing loaded into another process:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tests/tools/scan_host_check.cpp -o scan_host_check
//   ./scan_host_check <scratch directory>
// Exit code 0 and "scan host check ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <random>

#include "../../hammock_amd/csrc/hmk_scan.h"
#include "../../hammock_amd/host/hammock_targets.hpp"

using namespace hammock;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static std::string write(const std::string &dir, const std::string &name, const std::string &text) {
    const std::string path = dir + "/" + name;
    std::ofstream(path) << text;
    return path;
}

static bool refused(const std::string &path, const std::string &needle) {
    try {
        loadTargetsFromFasta(path, HMK_MAX_LEN + 1, HMK_TARGET_MAX_LEN);
    } catch (const TargetFormatError &e) {
        return std::string(e.what()).find(needle) != std::string::npos;
    }
    return false;
}

// the rule by brute force: every lane value a window can take, from the start value through every partial sum's extremes
static bool lanes_fit(int m, int X, int p, int thr, long long d, int bias, int max_m, long long bound) {
    if (m < hmk::SCAN_PACKED_MIN_LEN || m > hmk::SCAN_PACKED_MAX_LEN || X > hmk::SCAN_PACKED_MAX_SHIFT || max_m + bias > 255) return false;
    for (long long s = -X; s <= d + X; s += (s == 0 && d > 2 ? d : 1)) {   // the overhangs on both sides, the two ends of the interior
        const long long over = s < 0 ? -s : (s > d ? s - d : 0);
        const long long start = 128 - thr + d * p + 2 * p * over - (long long)bias * m;   // then m biased cells >= 0 each
        const long long top = 128 - thr + d * p + 2 * p * over + bound;
        if (start < 0 || top > 255) return false;
    }
    return true;
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    const std::string unit = "ACDEFGHIKLMNPQRSTVWY";
    {   // multi-line records, names cut at white space, lower case, blank lines, equal records kept apart
        const std::string path = write(dir, "targets_ok.fa", ">sp|P1 first protein\n" + unit + "\nacdefghiklmnpqrstvwy\n\n>two\tx\n" + unit + unit + "\n>three\r\n" +
                                                                 unit + "\r\n" + unit + "BZX*\r\n");
        const TargetSet set = loadTargetsFromFasta(path, HMK_MAX_LEN + 1, HMK_TARGET_MAX_LEN);
        EXPECT(set.size() == 3 && set.offsets.size() == 4);
        EXPECT(set.names[0] == "sp|P1" && set.names[1] == "two" && set.names[2] == "three");
        EXPECT(set.length(0) == 40 && set.length(1) == 40 && set.length(2) == 44);
        EXPECT(std::equal(set.residues.begin(), set.residues.begin() + 40, set.residues.begin() + 40));
        EXPECT(set.residues[set.offsets[2] + 40] == 20 && set.residues.back() == 23);
    }
    EXPECT(refused(write(dir, "targets_short.fa", ">long\n" + unit + unit + "\n>short one\n" + unit + unit.substr(0, 12) + "\n"), "\"short\""));
    EXPECT(refused(write(dir, "targets_short.fa", ">short\n" + unit + unit.substr(0, 12) + "\n"), "mode search"));
    EXPECT(refused(write(dir, "targets_letter.fa", ">a\n" + unit + unit + "\n>b\n" + unit + "J" + unit + "\n"), "'J'"));
    EXPECT(refused(write(dir, "targets_nohead.fa", unit + unit + "\n"), "header"));
    EXPECT(refused(dir + "/no_such_file.fa", "Cannot read"));
    {   // exactly the two limits pass, one more residue does not
        std::string big(HMK_TARGET_MAX_LEN, 'A');
        const TargetSet set = loadTargetsFromFasta(write(dir, "targets_limits.fa", ">min\n" + unit + unit.substr(0, 13) + "\n>max\n" + big + "\n"),
                                                   HMK_MAX_LEN + 1, HMK_TARGET_MAX_LEN);
        EXPECT(set.size() == 2 && set.length(0) == 33 && set.length(1) == HMK_TARGET_MAX_LEN);
        EXPECT(refused(write(dir, "targets_limits.fa", ">over\n" + big + "A\n"), "at most"));
    }
    EXPECT(loadTargetsFromFasta(write(dir, "targets_empty.fa", ""), HMK_MAX_LEN + 1, HMK_TARGET_MAX_LEN).size() == 0);

    // the class rule against the brute-force statement, over the parameters' ranges and beyond them
    std::mt19937 rng(7);
    long long checked = 0, fit = 0;
    for (int m = 4; m <= 22; m++)
        for (int X = 0; X <= 6 && X < m; X++)
            for (int p : {0, -1, -4, 1, 3, -300})
                for (int thr : {-30000, -5, 10, 20, 34, 120, 30000})
                    for (long long d : {1LL, 21LL, 52LL, 245LL, 1000LL, (long long)HMK_TARGET_MAX_LEN - m})
                        for (int bias : {0, 4, 1000})
                            for (int max_m : {11, 250, 1000}) {
                                const long long limit = hmk::scan_bound_limit(m, X, p, thr, d, bias, max_m);
                                EXPECT(limit >= -1);
                                for (int k = 0; k < 4; k++) {
                                    const long long bound = k == 0 ? 0 : k == 1 ? (limit < 0 ? 0 : limit) : k == 2 ? limit + 1 : (long long)(rng() % 400);
                                    const bool want = lanes_fit(m, X, p, thr, d, bias, max_m, bound);
                                    EXPECT((bound <= limit) == want);
                                    checked++;
                                    fit += want;
                                }
                            }
    EXPECT(fit > 0 && fit < checked);
    {   // the row bound: the best non-negative cell of every residue's row
        int32_t M[HMK_ALPHABET * HMK_ALPHABET];
        for (int a = 0; a < HMK_ALPHABET; a++)
            for (int b = 0; b < HMK_ALPHABET; b++) M[a * HMK_ALPHABET + b] = a == b ? a - 3 : -2;
        const uint8_t pep[6] = {0, 3, 5, 23, 2, 10};
        EXPECT(hmk::scan_row_bound(M, pep, 6) == 0 + 0 + 2 + 20 + 0 + 7);
    }
    if (failures) return 1;
    std::printf("scan host check ok (%lld rule cases, %lld of them fit)\n", checked, fit);
    return 0;
}
