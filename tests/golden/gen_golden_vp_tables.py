#!/usr/bin/env python3
"""Golden g27_vp_tables: the reference's own DDPM tables of the discrete VP score function -- captured by importing the reference
(read-only); run in the build container only:

    python tests/golden/gen_golden_vp_tables.py

For N in {8, 1000, 2000}: VPSDE(0.1, 20.0, N).discrete_betas and .sqrt_1m_alphas_cumprod (sde_lib.py:134-139), fp32 as the reference
holds them.  Only these arrays travel.  What they pin: the std the discrete score function divides by (utils.py:157-160), which the
kernels rebuild on the host (dposer_amd/csrc/sde_dev.h) -- N = 8 is the sampler's N of golden g26, 1000 the tasks', 2000 a table longer
than the network's 1000 sigmas.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden import ref_sde, save  # noqa: E402

NS = (8, 1000, 2000)


def main():
    out = {"N": np.asarray(NS, dtype=np.int64), "beta_min": np.float64(0.1), "beta_max": np.float64(20.0)}
    for n in NS:
        sde = ref_sde.VPSDE(0.1, 20.0, n)
        out[f"discrete_betas_{n}"] = sde.discrete_betas.numpy()
        out[f"sqrt_1m_alphas_cumprod_{n}"] = sde.sqrt_1m_alphas_cumprod.numpy()
        assert out[f"discrete_betas_{n}"].dtype == np.float32 and out[f"sqrt_1m_alphas_cumprod_{n}"].shape == (n,)
    save("g27_vp_tables", **out)


if __name__ == "__main__":
    main()
