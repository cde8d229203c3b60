// sizing_probe.cpp -- prints the values of hmk_sizing.h's functions for the inputs given on stdin, one call per line:
//   band n max_clusters | packed max_len min_len max_m shift_penalty max_shift threshold force_8byte |
//   guess symmetric n devices forced_guess have | overflow max_segment_count
// Each answer is the input line followed by " = value".  Host compiler only (tests/test_sizing.py builds and runs it).
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../hammock_amd/csrc/hmk_sizing.h"

int main() {
    using namespace hmk::sizing;
    std::printf("shards = %d\n", HMK_EDGE_SHARDS);
    char line[256];
    while (std::fgets(line, sizeof line, stdin)) {
        line[std::strcspn(line, "\n")] = 0;
        long long a[7];
        uint64_t u[5];
        if (std::sscanf(line, "band %lld %lld", &a[0], &a[1]) == 2)
            std::printf("%s = %lld\n", line, (long long)band_request((uint32_t)a[0], a[1]));
        else if (std::sscanf(line, "packed %lld %lld %lld %lld %lld %lld %lld", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6]) == 7)
            std::printf("%s = %d\n", line, (int)adjacency_packed((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4], (int)a[5], a[6] != 0));
        else if (std::sscanf(line, "guess %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &u[0], &u[1], &u[2], &u[3], &u[4]) == 5)
            std::printf("%s = %" PRIu64 "\n", line, edge_capacity_guess(u[0] != 0, (uint32_t)u[1], (uint32_t)u[2], u[3], u[4]));
        else if (std::sscanf(line, "overflow %" SCNu64, &u[0]) == 1)
            std::printf("%s = %" PRIu64 "\n", line, edge_capacity_after_overflow(u[0]));
        else {
            std::fprintf(stderr, "sizing_probe: cannot read '%s'\n", line);
            return 2;
        }
    }
    return 0;
}
