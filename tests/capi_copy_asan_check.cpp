// Host-side sanitizer run of msnake_copy_envs (msnake_capi.hip) WITHOUT a GPU: the checks that run before the first
// device call, under AddressSanitizer + UBSan (host code only: -fno-gpu-sanitize).  Without a device no handle can be
// created, so what is reachable is the handle validation: NULL handles and handles whose magic word is gone, which
// is what a destroyed handle looks like.  The stand-in for such a handle is a heap block of exactly four bytes, so
// that a read of anything behind the magic word before it has been checked is an ASan error.
// Built and run by tests/test_copy_envs_sanitizers.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../include/msnake.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "FAILED: %s (line %d): %s\n", #cond, __LINE__, msnake_last_error()); return 1; } \
    } while (0)

int main() {
    CHECK(msnake_abi_version() == MSNAKE_ABI_VERSION);
    uint32_t* word_a = static_cast<uint32_t*>(malloc(4));
    uint32_t* word_b = static_cast<uint32_t*>(malloc(4));
    CHECK(word_a && word_b);
    *word_a = 0u; *word_b = 0xDEADBEEFu;
    msnake_handle dead_a = reinterpret_cast<msnake_handle>(word_a), dead_b = reinterpret_cast<msnake_handle>(word_b);
    int32_t index[4] = {0, -1, 2, 99};   // a HOST array: never dereferenced, the call fails before any device work
    struct { msnake_handle dst, src; const int32_t* idx; } calls[] = {
        {nullptr, nullptr, nullptr}, {nullptr, nullptr, index}, {dead_a, nullptr, nullptr}, {nullptr, dead_a, index},
        {dead_a, dead_b, nullptr},   {dead_b, dead_a, index},   {dead_a, dead_a, nullptr},  {dead_b, dead_b, index},
    };
    for (auto& c : calls) {
        CHECK(msnake_copy_envs(c.dst, c.src, c.idx, nullptr) == MSNAKE_E_HANDLE);
        CHECK(strstr(msnake_last_error(), "handle") != nullptr);
    }
    // an odd index pointer changes nothing about the order: the handles are looked at first
    CHECK(msnake_copy_envs(dead_a, dead_b, reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(index) + 1), nullptr) ==
          MSNAKE_E_HANDLE);
    CHECK(*word_a == 0u && *word_b == 0xDEADBEEFu && index[3] == 99);   // nothing was written
    free(word_a); free(word_b);
    printf("CAPI COPY ASAN/UBSAN run clean\n");
    return 0;
}
