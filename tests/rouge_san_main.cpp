// A stand-alone driver of csrc_host/rouge.cpp for tests/test_rouge_host_cpu.py: built together with that file under
// AddressSanitizer + UndefinedBehaviorSanitizer, it reads one case dumped as raw little-endian files and prints one score per line as the
// hex of its float32 bits.
//   rouge_san <dir> <n_refs> <n_videos> <N> <Tc> <eos_id> <beta2 (a C hex float)> <n_threads>
//   <dir>/tokens.i32  <dir>/offsets.i64 [n_refs + 1]  <dir>/video_of_ref.i32 [n_refs]  <dir>/ids.i32 [N * Tc]  <dir>/video_of_row.i32 [N]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/s2vt_host.h"

template <typename T>
static std::vector<T> slurp(const std::string& path)
{
    std::vector<T> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(2); }
    T x;
    while (std::fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 9) { std::fprintf(stderr, "usage: see the head of rouge_san_main.cpp\n"); return 2; }
    const std::string dir = argv[1];
    const int n_refs = std::atoi(argv[2]), n_videos = std::atoi(argv[3]), N = std::atoi(argv[4]), Tc = std::atoi(argv[5]), eos = std::atoi(argv[6]);
    const double beta2 = std::strtod(argv[7], nullptr);
    const int n_threads = std::atoi(argv[8]);
    std::vector<int32_t> tokens = slurp<int32_t>(dir + "/tokens.i32"), vref = slurp<int32_t>(dir + "/video_of_ref.i32");
    std::vector<int64_t> offsets = slurp<int64_t>(dir + "/offsets.i64");
    std::vector<int32_t> ids = slurp<int32_t>(dir + "/ids.i32"), vrow = slurp<int32_t>(dir + "/video_of_row.i32");
    if ((int)offsets.size() != n_refs + 1 || (int)vref.size() != n_refs || (int)ids.size() != N * Tc || (int)vrow.size() != N ||
        (int64_t)tokens.size() != offsets[n_refs]) {
        std::fprintf(stderr, "the files do not match the sizes given\n");
        return 2;
    }
    s2vt_rouge* h = s2vt_rouge_create(tokens.data(), offsets.data(), vref.data(), n_refs, n_videos);
    if (!h) { std::fprintf(stderr, "s2vt_rouge_create failed\n"); return 3; }
    std::vector<float> out((size_t)N);
    const int rc = s2vt_rouge_score(h, ids.data(), N, Tc, eos, vrow.data(), beta2, out.data(), n_threads);
    s2vt_rouge_destroy(h);
    if (rc != 0) { std::fprintf(stderr, "s2vt_rouge_score returned %d\n", rc); return 4; }
    for (float x : out) {
        uint32_t bits;
        std::memcpy(&bits, &x, 4);
        std::printf("%08x\n", bits);
    }
    return 0;
}
