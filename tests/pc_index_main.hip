// Stand-alone host program of tests/test_pc_sampler_cpu.py: prints the table index that dposer_pc_sampler's launch code forms
// (dposer_amd/csrc/sde_dev.h, sde_table_index) for every fp32 time of a binary file: "<program> N T file" -> one index per line.
// No device code runs.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sde_dev.h"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const int N = atoi(argv[1]);
    const float T = (float)atof(argv[2]);
    FILE* f = fopen(argv[3], "rb");
    if (!f) return 3;
    float t;
    while (fread(&t, sizeof(float), 1, f) == 1) printf("%d\n", sde_table_index(t, N, T));
    fclose(f);
    return 0;
}
