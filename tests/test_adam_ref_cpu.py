"""The oracle of the training optimizer step (tests/adam_ref.py) is checked here before it judges the kernels
(tests/test_gpu_optimizer.py): its float64 run against torch.optim.Adam + clip_grad_norm_ + the EMA update over three chained steps, the
distance of its float32 run from its float64 run case by case (the band the GPU tolerance is 8 x of), and sharpness -- every planted
fault leaves that tolerance in at least one case."""
import numpy as np
import pytest
import torch

import adam_cases as AC
import adam_ref as AR


def test_float64_oracle_is_torch_adam_with_clip_and_ema():
    """Three chained steps from a preset step count, weight decay on, the clip active in the first step and idle in the last:
    torch.optim.Adam on a float64 parameter, torch.nn.utils.clip_grad_norm_ on the live tensor and s.sub_((1 - d) * (s - p)) against
    the float64 oracle, 1e-12 relative on every quantity."""
    rs = np.random.RandomState(7)
    n, step0, hyper = 1027, 4, dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, grad_clip=1.0, ema_one_minus_decay=0.25)
    p0, m0, v0 = rs.standard_normal(n), 0.1 * rs.standard_normal(n), 0.01 * rs.uniform(0.5, 1.5, n)
    s0 = p0 + 0.01 * rs.standard_normal(n)
    grads = [rs.standard_normal(n) * scale for scale in (1.0, 0.05, 0.01)]          # norms 32, 1.6, 0.32
    p = torch.nn.Parameter(torch.tensor(p0))
    opt = torch.optim.Adam([p], lr=hyper["lr"], betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"], weight_decay=hyper["weight_decay"])
    opt.state[p] = dict(step=torch.tensor(float(step0)), exp_avg=torch.tensor(m0), exp_avg_sq=torch.tensor(v0))
    s = torch.tensor(s0)
    st = dict(p=p0, m=m0, v=v0, s=s0)
    clipped = []
    for k, g in enumerate(grads, start=1):
        p.grad = torch.tensor(g)
        total = torch.nn.utils.clip_grad_norm_([p], hyper["grad_clip"])
        clipped.append(float(total) > hyper["grad_clip"])
        opt.step()
        with torch.no_grad():
            s.sub_(hyper["ema_one_minus_decay"] * (s - p))
        st = AR.adam_step(st["p"], g, st["m"], st["v"], st["s"], step=step0 + k, **hyper)
        assert not st["dropped"] and abs(st["sq"] - float(total) ** 2) <= 1e-12 * st["sq"]
        for name, got, want in (("p", st["p"], p.detach()), ("m", st["m"], opt.state[p]["exp_avg"]), ("v", st["v"], opt.state[p]["exp_avg_sq"]),
                                ("s", st["s"], s)):
            want = want.numpy()
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (k, name)
    assert clipped == [True, True, False] and int(opt.state[p]["step"]) == step0 + 3


def test_a_non_finite_squared_norm_drops_the_step():
    x = AC.inputs("clip_active")
    for bad in (np.nan, np.inf, -np.inf):
        g = np.array(x["g"])
        g[17] = bad
        out = AC.run_oracle("clip_active", state=dict(g=g))
        assert out["dropped"] and not np.isfinite(out["sq"])
        for k in ("p", "m", "v", "s"):
            assert np.array_equal(out[k], x[k].astype(np.float64))
    g = np.array(x["g"])
    g[17] = 1e20                    # finite, its float32 square is not
    assert AC.run_oracle("clip_active", dtype=np.float32, state=dict(g=g))["dropped"] and not AC.run_oracle("clip_active", state=dict(g=g))["dropped"]
    assert AC.run_oracle("clip_active", sq=np.inf)["dropped"]


def test_the_cases_are_the_cases_they_claim():
    for name, c in AC.CASES.items():
        x, ref, h = AC.inputs(name), AC.reference(name), c["hyper"]
        n = c["n"]
        assert all(a is None or (a.dtype == np.float32 and a.shape == (n,)) for a in x.values()) and (x["s"] is None) == (not c["ema"])
        tiny = np.finfo(np.float32).tiny
        for k in ("p", "g", "m", "v", "s"):               # float32 inputs and float64 results: zero or normal
            for a in (x[k], ref[k] if k != "g" else None):
                assert a is None or (np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= tiny * 1e3)).all()), (name, k)
        g64 = x["g"].astype(np.float64)
        assert name == "two_trips" or (g64[-min(3, n):] ** 2).sum() > 0.2 * ref["sq"], name          # the tail of the norm matters
        assert not ref["dropped"] and abs(ref["sq"] - (g64 ** 2).sum()) <= 1e-14 * ref["sq"]
        norm = np.sqrt(ref["sq"]) * h["grad_scale"]
        for lo, hi in c["skips"]:
            assert 0 <= lo < hi <= n and (x["g"][lo:hi] == 0).all() and (x["m"][lo:hi] != 0).all()
            assert np.array_equal(ref["p"][lo:hi], x["p"][lo:hi]) and np.array_equal(ref["m"][lo:hi], x["m"][lo:hi]) and (ref["s"][lo:hi] != x["s"][lo:hi]).all()
        if name in ("clip_active", "no_ema", "weight_decay_clip", "grad_scale", "two_trips", "model_d63") or name[1:].isdigit():
            assert norm > 5 * h["grad_clip"] > 0, (name, norm)
        if name == "first_step":
            assert norm < h["grad_clip"] and h["step"] == 1 and not x["m"].any() and not x["v"].any() and np.array_equal(x["s"], x["p"])
        if name == "tiny_clip":
            assert 1e-3 < norm < 1e-2 and h["grad_clip"] == 1e-3
        if name == "skips":
            assert all(lo % 4 and hi % 4 for lo, hi in c["skips"]) and len(c["skips"]) == 2
        if name == "two_trips":
            assert n == 2 ** 20 + 7 and (g64[AR.TRIP:] ** 2).sum() > 0.1 * ref["sq"]
    assert AC.MODEL_N == 1070783 and AC.MODEL_COND == (98816, 361472)


def test_float32_oracle_stays_inside_the_band():
    """Every case in float32 against float64, quantity by quantity: the table of D32.  A fresh measurement stays within 2 x of every
    recorded constant (and the constants were not inflated: what is recorded is what is measured, to the digits written down)."""
    print()
    for name in AC.CASES:
        ref, x = AC.reference(name), AC.inputs(name)
        d = AC.distances(AC.run_oracle(name, np.float32), ref, x)
        print(f'    "{name}": dict(' + ", ".join(f"{q}={v:.2e}" for q, v in d.items()) + "),")
        assert set(d) == set(AC.D32_MEASURED[name]), name
        for q, v in d.items():
            rec = AC.D32_MEASURED[name][q]
            assert v <= 2 * max(rec, AC.FLOOR), (name, q, v, rec)
            assert rec <= 2 * max(v, AC.FLOOR), (name, q, v, rec)
            assert v < AC.TOL[name][q]


# mutation -> the cases it is looked for in (None: every case of 1027 elements and the small sizes)
ONLY_IN = {"second_trip_missing_from_norm": ("two_trips",), "second_trip_untouched": ("two_trips",)}


@pytest.mark.parametrize("mutation", AR.MUTATIONS)
def test_a_planted_fault_leaves_the_band(mutation):
    """A kernel with this defect could not pass the GPU comparison: planted into the float64 oracle it moves a compared quantity of at
    least one case out of that case's tolerance (8 x D32)."""
    caught = []
    for name in ONLY_IN.get(mutation, AC.CASES):
        d = AC.distances(AC.run_oracle(name, mutation=mutation), AC.reference(name), AC.inputs(name))
        q = max(d, key=lambda k: d[k] / AC.TOL[name][k])
        if d[q] > AC.TOL[name][q]:
            caught.append((d[q] / AC.TOL[name][q], name, q))
    caught.sort(reverse=True)
    print(f"\n{mutation}: " + (", ".join(f"{name}.{q} {r:.3g} x tol" for r, name, q in caught[:4]) or "NOT CAUGHT") + f" ({len(caught)} cases)")
    assert caught, mutation
