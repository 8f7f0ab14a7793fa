// Stand-alone check of the host half of amd_ivf_build_dev (auncel_amd/csrc/build_args.h): every refusal that is made before anything
// is launched, in the order the call reports them, and the cut of the second sweep into chunks.  Built with
// -fsanitize=address,undefined and run directly (tests/test_build_dev_cpu.py).
#include <cstdio>

#include "../../auncel_amd/csrc/build_args.h"

using namespace amdivf;

static int failures = 0;
// `change` applied to a call that is in order: the refusal names `what` (empty: no refusal)
#define CASE(change, what) do { BuildArgs a = good; change; const std::string e = build_args_error(a);                      \
    if (*what ? e.find(what) == std::string::npos : !e.empty()) failures += printf("FAILED line %d: \"%s\", not \"%s\"\n", __LINE__, e.c_str(), what) > 0; } while (0)
#define CHUNK(n, nlist, forced, want) failures += build_chunk_tiles(n, nlist, 1024, BUILD_CHUNK_BYTES, forced) != want ? (printf("FAILED line %d\n", __LINE__), 1) : 0

int main() {
    alignas(16) static char mem[64];
    const void *p = mem, *four = mem + 4, *two = mem + 2;
    const BuildArgs good{true, true, false, true, 5, 8, p, DEV_PTR_DEVICE, 0, 8, p, DEV_PTR_DEVICE, p, DEV_PTR_DEVICE};
    CASE((void)0, "");
    CASE(a.ids = a.assign = nullptr, "");  // (both are optional)
    CASE(a.have_handle = false, "build_dev: null argument");
    CASE(a.have_out = false, "build_dev: null argument");
    CASE(a.is_clone = true, "amd_ivf_clone");
    CASE(a.have_centroids = false, "no centroids");
    CASE((a.have_centroids = false, a.is_clone = true), "amd_ivf_clone");  // (the order of the report)
    CASE(a.dtype = 2, "dtype");
    CASE(a.ldx = 7, "ldx");
    CASE(a.x = nullptr, "d_x: null pointer");
    CASE(a.kind_x = DEV_PTR_HOST, "d_x: not a device pointer");
    CASE(a.kind_x = DEV_PTR_OTHER_DEVICE, "d_x: device memory of another device");
    CASE(a.x = two, "d_x: misaligned");
    CASE((a.x = two, a.dtype = 1), "");  // (aligned for fp16)
    CASE(a.kind_ids = DEV_PTR_HOST, "d_ids: not a device pointer");
    CASE(a.kind_ids = DEV_PTR_OTHER_DEVICE, "d_ids: device memory of another device");
    CASE(a.ids = four, "d_ids: misaligned");
    CASE(a.kind_assign = DEV_PTR_UNKNOWN, "d_assign: not a device pointer");
    CASE(a.assign = four, "d_assign: misaligned");
    CASE((a.ids = nullptr, a.kind_ids = DEV_PTR_UNKNOWN), "");  // (an absent array has no kind)
    CASE((a.n = 0, a.x = nullptr, a.kind_x = DEV_PTR_UNKNOWN, a.kind_ids = DEV_PTR_HOST, a.dtype = 7), "");
    CASE((a.n = 0, a.have_centroids = false), "no centroids");
    // chunks: whole tiles within the 64 MiB budget, at least one, at most all; the tests' switch in rows, rounded down to tiles
    CHUNK(10000000, 4096, 0, 4096);
    CHUNK(10000000, 16, 0, 9766);       // (all of them)
    CHUNK(10000000, 1u << 30, 0, 1);  // (a row of counts above the budget: a tile a chunk)
    CHUNK(0, 16, 0, 1);
    CHUNK(2049, 16, 1024, 1);
    CHUNK(5000, 16, 2500, 2);
    CHUNK(2049, 16, 1u << 20, 3);
    printf(failures ? "%d check(s) failed\n" : "DONE\n", failures);
    return failures != 0;
}
