// key_path_hash.cpp — TEST-ONLY (tests/test_key_path_cpu.py compiles and runs it): the hashes of gubernator_amd/csrc/guber_algo.h on the
// host.  Reads lines "<len> <hex of 32 bytes>" and prints, per line, xxhash64 of the first len bytes, xxhash64_words4 and
// xxhash64_words4_uniform of the four words the 32 bytes make — the bytes behind the key are whatever the caller put there.
#include <cstdio>
#include <cstring>

#include "../../gubernator_amd/csrc/guber_algo.h"

int main() {
    char hex[128];
    unsigned len = 0;
    while (scanf("%u %127s", &len, hex) == 2) {
        if (len >= 32 || strlen(hex) != 64) return 2;
        uint8_t b[32];
        for (int i = 0; i < 32; ++i) { unsigned v = 0; if (sscanf(hex + 2 * i, "%2x", &v) != 1) return 2; b[i] = (uint8_t)v; }
        uint64_t w[4];
        memcpy(w, b, 32);
        printf("%llu %llu %llu\n", (unsigned long long)guber::xxhash64(b, len, 0), (unsigned long long)guber::xxhash64_words4(w, len, 0),
               (unsigned long long)guber::xxhash64_words4_uniform(w, len, 0));
    }
    return 0;
}
