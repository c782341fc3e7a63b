"""What the five optimizer entries of the C ABI refuse, without a GPU: every case is refused by an argument check, so nothing is
launched -- the return code is DPOSER_ERR_BAD_ARG (a launch attempt on this machine would come back as DPOSER_ERR_HIP), the message keeps
its words, and it starts with the name of the extern "C" entry that was called (not with the name of the body three entries share)."""
import ctypes as C

import pytest

from dposer_amd import _C

BAD_ARG = -1
FAKE = C.c_void_p(0x1000)              # a 256-byte aligned "device pointer": a refused call never dereferences it
ALIGNED_16 = C.c_void_p(0x1010)        # 16-byte aligned only
ALIGNED_4 = C.c_void_p(0x1004)         # a float boundary that is no float4 boundary
N = 1000
HYPER = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_clip=1.0, grad_scale=1.0)

PLAIN = ("dposer_adam_ema_clip_step", "dposer_adam_ema_clip_step_wd", "dposer_adam_ema_clip_step_presummed")
PACK, SQNORM = "dposer_scorefc_adam_pack_step", "dposer_grad_sqnorm"
BUFFERS = ("flat", "grad", "m", "v", "scratch")


def _i64x2(a):
    return None if a is None else (C.c_int64 * 2)(*a)


def _args(entry, o):
    """The argument list of ``entry`` from the overrides ``o``; the defaults are a well-formed call (which would launch: never made here)."""
    g = lambda k, d=FAKE: o.get(k, d)
    n_skip = g("n_skip", 1)
    lo, hi = _i64x2(g("lo", (4, 0))), _i64x2(g("hi", (12, 0)))
    h = [HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"]]
    tail = [HYPER["grad_clip"], HYPER["grad_scale"], g("adam_step", 1), 0.1, g("scratch")]
    if entry == SQNORM:
        return [g("grad"), g("n", N), g("scratch"), None]
    if entry == PACK:
        return [g("h"), g("flat"), g("grad"), g("m"), g("v"), g("ema"), g("packed"), lo, hi, n_skip] + h + [HYPER["weight_decay"]] + tail + [0, None]
    head = [g("flat"), g("grad"), g("m"), g("v"), g("ema"), g("n", N), lo, hi, n_skip] + h
    if entry == "dposer_adam_ema_clip_step_wd":
        return head + [HYPER["weight_decay"]] + tail + [g("presummed", 0), None]
    return head + tail + [None]


def _cases():
    cases = []          # (entry, what, overrides, text)
    for e in PLAIN:
        for b in BUFFERS:
            cases.append((e, f"null {b}", {b: None}, "null argument"))
        cases.append((e, "n -1", {"n": -1}, "n must be >= 0"))
        cases.append((e, "misaligned grad", {"grad": ALIGNED_4}, "grad must be 16-byte aligned"))
    for e in PLAIN + (PACK,):
        cases.append((e, "adam_step 0", {"adam_step": 0}, "adam_step counts from 1"))
        for k in (3, -1):
            cases.append((e, f"n_skip {k}", {"n_skip": k}, "at most two no-gradient ranges"))
        cases.append((e, "null skip_lo", {"lo": None}, "null argument"))
        cases.append((e, "null skip_hi", {"hi": None}, "null argument"))
        cases.append((e, "range below 0", {"lo": (-1, 0)}, "a no-gradient range must satisfy 0 <= lo <= hi <= n"))
        cases.append((e, "range lo above hi", {"lo": (13, 0)}, "a no-gradient range must satisfy 0 <= lo <= hi <= n"))
        cases.append((e, "range beyond n", {"hi": (1 << 40, 0)}, "a no-gradient range must satisfy 0 <= lo <= hi <= n"))
        cases.append((e, "second range beyond n", {"n_skip": 2, "lo": (4, 20), "hi": (12, 1 << 40)}, "a no-gradient range must satisfy 0 <= lo <= hi <= n"))
    cases.append((PLAIN[1], "range ends at n + 1", {"hi": (N + 1, 0)}, "a no-gradient range must satisfy 0 <= lo <= hi <= n"))
    for b in ("h",) + BUFFERS + ("packed",):
        cases.append((PACK, f"null {b}", {b: None}, "null argument"))
    for b in ("flat", "grad", "m", "v", "ema"):
        cases.append((PACK, f"misaligned {b}", {b: ALIGNED_4}, "buffers must be 16-byte aligned (packed: 256)"))
    cases.append((PACK, "packed aligned to 16 only", {"packed": ALIGNED_16}, "buffers must be 16-byte aligned (packed: 256)"))
    cases.append((PACK, "bf16x3 handle", {"h": "x3"}, "fused optimizer + re-pack step not available for this configuration"))
    cases.append((SQNORM, "null grad", {"grad": None}, "bad argument"))
    cases.append((SQNORM, "null scratch", {"scratch": None}, "bad argument"))
    cases.append((SQNORM, "n -1", {"n": -1}, "bad argument"))
    cases.append((SQNORM, "misaligned grad", {"grad": ALIGNED_4}, "grad must be 16-byte aligned"))
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def handles():
    lib = _C.lib()
    out = {}
    for name, prec in (("h", _C.PREC_BF16), ("x3", _C.PREC_BF16X3)):
        h = C.c_void_p()
        d = _C.ScoreFCDesc(63, 512, 128, 1, _C.EMB_POSITIONAL, 1, 1000, prec, 0.1)
        assert lib.dposer_scorefc_create(C.byref(d), C.byref(h)) == 0
        out[name] = h
    yield out
    for h in out.values():
        lib.dposer_scorefc_destroy(h)


def test_the_table_covers_the_five_entries():
    assert all(name in _C.SIGNATURES for name in PLAIN + (PACK, SQNORM))
    assert {c[0] for c in CASES} == set(PLAIN + (PACK, SQNORM))
    for e in PLAIN + (PACK, SQNORM):
        assert len(_args(e, {"h": FAKE})) == len(_C.SIGNATURES[e][1]), e
    for e in PLAIN + (PACK,):
        whats = [w for (entry, w, *_rest) in CASES if entry == e]
        assert {"null flat", "adam_step 0", "n_skip 3", "range beyond n"} <= set(whats), e


@pytest.mark.parametrize("entry,what,over,text", CASES, ids=[f"{c[0]}-{c[1].replace(' ', '_')}" for c in CASES])
def test_refusal(handles, entry, what, over, text):
    lib = _C.lib()
    o = {"h": handles["h"]}
    o.update(over)
    if o["h"] == "x3":
        o["h"] = handles["x3"]
    rc = getattr(lib, entry)(*_args(entry, o))
    msg = lib.dposer_last_error().decode()
    assert rc == BAD_ARG, (rc, msg)
    assert text in msg, msg
    assert msg.startswith(entry + ": "), msg
