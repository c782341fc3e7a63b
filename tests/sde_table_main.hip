// Stand-alone host program of tests/test_sde_ref_cpu.py: prints the discrete-VP std table that the kernels' launch code forms
// (dposer_amd/csrc/sde_dev.h, sde_vp_sqrt_1m_alphas_cumprod / make_sde_dev_at) as "N k bits" lines, for every N on the command line.
// No device code runs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include "sde_dev.h"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        SdeCfg c;
        c.kind = SDE_VP; c.discrete = 1; c.beta_0 = 0.1; c.beta_1 = 20.0; c.N = atoi(argv[a]); c.T = 1.0f;
        for (int k = 0; k < c.N; ++k) {
            // through the launch path's own entry: the t whose index is k (t (N - 1) truncates to k for t = (k + 0.5) / (N - 1))
            const float t = c.N > 1 ? ((float)k + 0.5f) / (float)(c.N - 1) : 0.f;
            const float direct = sde_vp_sqrt_1m_alphas_cumprod(c, k), at = make_sde_dev_at(c, t).sd_disc;
            uint32_t b0, b1;
            memcpy(&b0, &direct, 4); memcpy(&b1, &at, 4);
            printf("%d %d %08x %08x\n", c.N, k, b0, b1);
        }
    }
    return 0;
}
