// TEST INFRASTRUCTURE: reads a medium JSON from stdin through the stand-alone host adapter (libgpis_host.so) and prints what a
// tabulated mean reads of the two mean slots of the gpis_params it yields, or "error: <message>"
// (tests/test_grid_mean_json_cpu.py).  No GPU is touched: fromJson only.
#include <cstdio>
#include <exception>
#include <iostream>
#include <iterator>
#include <string>

#include "HipSparseConvNoiseMedium.hpp"

static void print_mean(const char *name, const gpis_mean &m)
{
    std::printf("%s type=%d volume=%d offset=%.9g scale=%.9g\n", name, m.type, m.func, (double)m.offset, (double)m.scale);
}

int main()
{
    std::string json((std::istreambuf_iterator<char>(std::cin)), std::istreambuf_iterator<char>());
    gpis_host::HipSparseConvNoiseMedium medium;
    try {
        medium.fromJson(json);
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 0;
    }
    const gpis_params &p = medium.params();
    print_mean("mean", p.mean);
    std::printf("has_mean_additional=%d\n", p.has_mean_additional);
    print_mean("mean_additional", p.mean_additional);
    return 0;
}
