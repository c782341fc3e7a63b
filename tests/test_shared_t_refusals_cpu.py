"""What the 14 shared-t entry points of the C ABI refuse, without a GPU: every case is refused by an argument check, so nothing is
launched -- the return code is DPOSER_ERR_BAD_ARG or DPOSER_ERR_UNSUPPORTED (a launch attempt on this machine would come back as
DPOSER_ERR_HIP), the message keeps its words, and it starts with the name of the extern "C" entry that was called (not with the
name of a body several entries share)."""
import ctypes as C

import pytest

from dposer_amd import _C

BAD_ARG, UNSUPPORTED = -1, -2
FAKE = C.c_void_p(0x1000)              # a 256-byte aligned "device pointer": a refused call never dereferences it
MISALIGNED = C.c_void_p(0x1010)        # 16-byte aligned only
TIMES = (C.c_float * 66)(*[1.0 - i / 80.0 for i in range(66)])       # host arrays are real: strictly decreasing inside (0, T]
ONES_F = (C.c_float * 66)(*([1.0] * 66))
ONES_I = (C.c_int32 * 66)(*([1] * 66))


def _sde(kind=_C.SDE_SUBVP):
    return C.byref(_C.SdeDesc(kind, 1000, 0.1, 20.0, 1.0))


def _pc():
    return C.byref(_C.PcDesc(_C.PC_PRED_EULER_MARUYAMA, _C.PC_CORR_NONE, 0, 0, 0.16, 1.0))


# entry -> argument list from the overrides `o`; the defaults are a well-formed call (which would launch: never made here)
def _em(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], FAKE, FAKE, TIMES, 0, o.get("obs"), o.get("mask"), None, 0, None, o.get("traj_stride", 1), FAKE,
            FAKE, 16, None]


def _em_steps(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], FAKE, FAKE, TIMES, 0, 3, o.get("obs"), o.get("mask"), None, 0, None, o.get("traj_stride", 1),
            FAKE, FAKE, 16, None]


def _pc_sampler(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], _pc(), FAKE, FAKE, TIMES, 0, 3, o.get("obs"), o.get("mask"), None, 0, None,
            o.get("traj_stride", 1), None, None, FAKE, FAKE, 16, None]


def _dpm(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], C.byref(_C.DpmDesc(o.get("order", 2), 1)), FAKE, FAKE, FAKE, TIMES, 3, o.get("obs"), o.get("mask"),
            None, 0, None, o.get("traj_stride", 1), FAKE, FAKE, 16, None]


def _guided(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], FAKE, FAKE, TIMES, 0, 3, o.get("obs", FAKE), o.get("mask", FAKE), None, 0, None,
            o.get("traj_stride", 1), o.get("project", 0), 1.0, FAKE, FAKE, FAKE, 16, None]


def _langevin(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], FAKE, FAKE, 0.5, 1.0, 0.16, None, 0, 0, FAKE, o.get("phase", 0), 1.0, FAKE, FAKE, 16, None]


def _prior_loss(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], FAKE, None, 0.3, 1, 1.0, FAKE, FAKE, FAKE, 0, 0, FAKE, FAKE, 16, None]


def _table_build(o):
    return [o["h"], FAKE, FAKE, o["ws"], TIMES, 3, FAKE, 16, None]


def _table_build_sde(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], TIMES, 3, FAKE, 16, None]


def _prior_loss_tabled(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], FAKE, None, 0.3, 0, 3, 1, 1.0, FAKE, FAKE, FAKE, 0, 0, FAKE, 16, None]


def _prior_loss_multi(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], FAKE, None, TIMES, o.get("n_steps", 5), 1, 1.0, FAKE, FAKE, FAKE, 0, 0, FAKE, FAKE, 16, None]


def _red_diff(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], FAKE, None, 0.3, 1.0, FAKE, FAKE, FAKE, 0, 0, FAKE, FAKE, 16, None]


def _completion(o):
    return [o["h"], FAKE, FAKE, o["ws"], o["sde"], FAKE, FAKE, FAKE, FAKE, FAKE, TIMES, ONES_I, ONES_F, ONES_F, 3, 0.1, 0.9, 0.999, 1e-8, None, 0,
            0, FAKE, FAKE, 16, None]


ENTRIES = {
    "dposer_pc_sampler": _pc_sampler, "dposer_em_sampler": _em, "dposer_pf_sampler": _em, "dposer_em_sampler_steps": _em_steps,
    "dposer_dpm_sampler": _dpm, "dposer_langevin_step": _langevin, "dposer_prior_loss": _prior_loss, "dposer_prior_loss_tabled": _prior_loss_tabled,
    "dposer_prior_table_build": _table_build, "dposer_prior_table_build_sde": _table_build_sde, "dposer_prior_loss_multi": _prior_loss_multi,
    "dposer_prior_red_diff": _red_diff, "dposer_completion_optimize": _completion, "dposer_guided_sampler": _guided,
}
NO_SDE = ("dposer_prior_table_build",)                       # takes no descriptor
SDE_OPTIONAL = ("dposer_prior_table_build_sde",)             # null: the labels t * 999 of dposer_prior_table_build
LOOPS = ("dposer_pc_sampler", "dposer_em_sampler", "dposer_pf_sampler", "dposer_em_sampler_steps", "dposer_dpm_sampler")
UNKNOWN_KIND = {"dposer_guided_sampler": "the guided sampler takes the continuous sub-VP and VP score functions"}
CONTINUOUS_ONLY = "continuous score functions only (sub-VP, VP, VE)"


def _cases():
    cases = []          # (entry, what, overrides, code, text)
    for e in ENTRIES:
        cases.append((e, "null handle", {"h": None}, BAD_ARG, "null argument"))
        if e not in NO_SDE + SDE_OPTIONAL:
            cases.append((e, "null sde", {"sde": None}, BAD_ARG, "null argument"))
        if e not in NO_SDE:
            cases.append((e, "sde kind 9", {"sde": _sde(9)}, BAD_ARG, UNKNOWN_KIND.get(e, "unknown SDE kind")))
        cases.append((e, "misaligned workspace", {"ws": MISALIGNED}, BAD_ARG, "packed / workspace must be 256-byte aligned"))
    for n in (0, 65):
        cases.append(("dposer_prior_loss_multi", f"n_steps {n}", {"n_steps": n}, BAD_ARG, "n_steps must be in 1..64"))
    for kind, name in ((_C.SDE_VE_DISCRETE, "VE discrete"), (_C.SDE_VP_DISCRETE, "VP discrete")):
        cases.append(("dposer_prior_loss_multi", name, {"sde": _sde(kind)}, BAD_ARG, CONTINUOUS_ONLY))
        cases.append(("dposer_prior_red_diff", name, {"sde": _sde(kind)}, BAD_ARG, CONTINUOUS_ONLY))
        cases.append(("dposer_dpm_sampler", name, {"sde": _sde(kind)}, UNSUPPORTED, CONTINUOUS_ONLY))
    for e in LOOPS:
        cases.append((e, "observation without mask", {"obs": FAKE, "mask": None}, BAD_ARG, "observation and mask go together"))
    cases.append(("dposer_guided_sampler", "observation without mask", {"obs": FAKE, "mask": None}, BAD_ARG, "observation and mask are required"))
    for e in LOOPS + ("dposer_guided_sampler",):
        cases.append((e, "traj_stride 0", {"traj_stride": 0}, BAD_ARG, "traj_stride must be >= 1"))
    cases.append(("dposer_guided_sampler", "project 2", {"project": 2}, BAD_ARG, "project must be 0 (DPS) or 1 (MCG)"))
    cases.append(("dposer_langevin_step", "phase 2", {"phase": 2}, BAD_ARG, "phase must be 0 (norms) or 1 (update)"))
    cases.append(("dposer_dpm_sampler", "order 3", {"order": 3}, BAD_ARG, "order must be 1 or 2"))
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def handle():
    lib = _C.lib()
    h = C.c_void_p()
    d = _C.ScoreFCDesc(63, 1024, 512, 2, _C.EMB_POSITIONAL, 1, 1000, _C.PREC_FP32, 0.1)
    assert lib.dposer_scorefc_create(C.byref(d), C.byref(h)) == 0
    yield h
    lib.dposer_scorefc_destroy(h)


def test_the_table_covers_the_fourteen_entries():
    assert len(ENTRIES) == 14 and all(name in _C.SIGNATURES for name in ENTRIES)
    for e in ENTRIES:
        whats = [w for (entry, w, *_rest) in CASES if entry == e]
        assert "null handle" in whats and "misaligned workspace" in whats
        assert ("null sde" in whats) == (e not in NO_SDE + SDE_OPTIONAL) and ("sde kind 9" in whats) == (e not in NO_SDE)


@pytest.mark.parametrize("entry,what,over,code,text", CASES, ids=[f"{c[0]}-{c[1].replace(' ', '_')}" for c in CASES])
def test_refusal(handle, entry, what, over, code, text):
    lib = _C.lib()
    o = {"h": handle, "ws": FAKE, "sde": _sde()}
    o.update(over)
    rc = getattr(lib, entry)(*ENTRIES[entry](o))
    msg = lib.dposer_last_error().decode()
    assert rc == code, (rc, msg)
    assert text in msg, msg
    assert msg.startswith(entry + ": "), msg
