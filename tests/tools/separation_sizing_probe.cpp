// separation_sizing_probe.cpp -- prints hmk_sizing.h's separation_segments for the inputs given on stdin, one call per line:
//   <members> <forced segment length>
// Each answer is the input line followed by " = <segment length> <segments>".  Host compiler only (tests/test_separation.py builds
// and runs it).
#include <cstdio>
#include <cstring>

#include "../../hammock_amd/csrc/hmk_sizing.h"

int main() {
    using namespace hmk::sizing;
    std::printf("limits = %u %u %u\n", SEPARATION_ITEMS, SEPARATION_MAX_SEGMENTS, SEPARATION_MIN_SEGMENT);
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        line[std::strcspn(line, "\n")] = 0;
        unsigned nm, forced;
        if (std::sscanf(line, "%u %u", &nm, &forced) != 2) {
            std::fprintf(stderr, "separation_sizing_probe: cannot read '%s'\n", line);
            return 2;
        }
        const SeparationSegments s = separation_segments(nm, forced);
        std::printf("%s = %u %u\n", line, s.length, s.count);
    }
    return 0;
}
