// The five-point solver of csrc/metrics.hip on the host: essential_poly and essential_roots are __host__ __device__, so the same
// text runs here without a GPU.  tests/test_metrics_cases_cpu.py compiles this (host side only), feeds it the crafted families of
// tests/metrics_cases.py and compares with the numpy restatement.  The host path may contract differently from the device path; the
// GPU tests remain the judge of the kernels.
//   five_point_host IN OUT     IN: int32 count, x0 [count][5][2], x1 [count][5][2] doubles.  OUT: int32 ns [count], E [count][90] doubles.
#include "../../openglue_amd/csrc/metrics.hip"

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t count = 0;
    if (fread(&count, 4, 1, f) != 1 || count <= 0 || count > (1 << 20)) return 4;
    std::vector<double> x0((size_t)count * 10), x1((size_t)count * 10), E((size_t)count * kSlots, 0.0);
    std::vector<int32_t> ns(count);
    if (fread(x0.data(), 8, x0.size(), f) != x0.size() || fread(x1.data(), 8, x1.size(), f) != x1.size()) return 5;
    fclose(f);
    std::vector<double> A(200);
    for (int p = 0; p < count; ++p) {
        double* slot = E.data() + (size_t)p * kSlots;      // as in the kernels: the intermediate state lives in the output slots
        essential_poly(&x0[(size_t)p * 10], &x1[(size_t)p * 10], A.data(), 1, slot, 1);
        ns[p] = essential_roots(slot, 1, slot);
    }
    f = fopen(argv[2], "wb");
    if (!f) return 6;
    fwrite(ns.data(), 4, ns.size(), f);
    fwrite(E.data(), 8, E.size(), f);
    fclose(f);
    return 0;
}
