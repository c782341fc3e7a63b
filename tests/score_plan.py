"""``dposer_scorefc_plan`` for the tests: which GEMM tiling and launch form a batch takes under the tuning loaded, and the forced
policies that put the large-batch tilings onto batches an oracle can check.  A test that forces a tiling asserts through ``plan`` that
the forcing took: a later change of the policy functions then fails that assertion instead of re-routing the test silently."""
import collections
import ctypes as C

from dposer_amd import _C

# gemm_api.h
BIG, MID, SMALL, FINAL, FINAL_S, WIDE64, SMALL64 = range(7)      # 256x256, 128x128, 128x32, 64x128, 64x32, 128x64 (4 waves), 128x64 (8 waves)
# weight-gradient forms
SPLIT_K, ONE_LAUNCH, LANE_GROUPS = 0, 1, 2

Plan = collections.namedtuple("Plan", "padded gn gn_bwd time final wgrad wgrad_form groups time_split side_stream")

# Every switch that keeps a small batch on the small-batch tilings is lifted; what is left decides between 256x256 and 128x128.
POLICY_BIG = dict(DPOSER_SMALL_TILE_MAX="0", DPOSER_BIG_MIN_BATCH="256", DPOSER_GNBWD_BIG="1", DPOSER_WGRAD_BIG="1", DPOSER_FINAL_SMALL_MAX="0")
POLICY_MID = dict(DPOSER_SMALL_TILE_MAX="0", DPOSER_GNBWD_BIG="0", DPOSER_WGRAD_BIG="0", DPOSER_FINAL_SMALL_MAX="0")
POLICIES = {"default": {}, "MID": POLICY_MID, "BIG": POLICY_BIG}
SWITCHES = ("DPOSER_SMALL_TILE_MAX", "DPOSER_BIG_MIN_BATCH", "DPOSER_GNBWD_BIG", "DPOSER_WGRAD_BIG", "DPOSER_FINAL_SMALL_MAX", "DPOSER_WGRAD_BATCHED",
            "DPOSER_SILU_SPLIT_MAX")
GEMM_OF = {"default": SMALL, "MID": MID, "BIG": BIG}             # the tiling of the GroupNorm layers and the time branch under a policy (swish)


def force(tuning_env, policy, **extra):
    """Load a policy of POLICIES (plus ``extra`` switches) through the ``tuning_env`` fixture; every switch it does not name is cleared."""
    env = {k: None for k in SWITCHES}
    env.update(POLICIES[policy])
    env.update(extra)
    tuning_env(**env)


def plan(h, B, events=False):
    """The plan of handle ``h`` (a ``dposer_scorefc_t``) for a batch of B samples; ``events``: the bucketed backward with bucket events."""
    out = (C.c_int32 * 10)()
    rc = _C.lib().dposer_scorefc_plan(h, B, 1 if events else 0, out)
    assert rc == 0, _C.lib().dposer_last_error()
    return Plan(*out)


def model_plan(m, B, events=False):
    return plan(m._engine().h, B, events)


def make_handle(H=1024, precision="bf16", activation="swish", D=63, E=512, n_blocks=2):
    h = C.c_void_p()
    d = _C.ScoreFCDesc(D, H, E, n_blocks, _C.EMB_POSITIONAL, 1, 1000, _C.PRECISIONS[precision], 0.1, _C.ACTIVATIONS[activation])
    assert _C.lib().dposer_scorefc_create(C.byref(d), C.byref(h)) == 0, _C.lib().dposer_last_error()
    return h
