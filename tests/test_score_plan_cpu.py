"""``dposer_scorefc_plan`` (host only): which tiling and launch form the score network takes for a batch.

The GPU tests hold the large-batch tilings to an oracle by forcing them onto small batches through the DPOSER_* switches.  The forcing
can only be trusted if it can be observed: these tests pin the default policy to a table written out from the documented thresholds
(``ScoreTuning`` in csrc/scorefc.hip, include/dposer_hip.h), and every forced policy a GPU test uses to the tiling that test names.
Whoever moves a threshold edits the table below and sees here which GPU tests lean on it."""
import os

import pytest

import score_plan as SP
from score_plan import BIG, FINAL, FINAL_S, MID, SMALL, SMALL64
from dposer_amd import _C

BATCHES = [1, 64, 65, 200, 512, 513, 1024, 1025, 2048, 2049, 2304, 4096, 4097, 8192, 16384, 16385, 32768, 32769, 65536]
PRECISIONS = ("bf16", "fp32", "bf16x3")

# The default policy, from the documented thresholds:
#   padding        to 64 samples up to 512, to 256 above
#   GroupNorm      forward and dgrad: 128x32 up to 2048 padded samples (DPOSER_SMALL_TILE_MAX), 128x128 above, 256x256 from 16384 (DPOSER_BIG_MIN_BATCH;
#                  the dgrad's own crossover is 16384 as well) -- 256x256 only for 32-channel groups (hidden 1024) and swish;
#                  bf16 storage, hidden 1024, swish: 128x64 on eight waves for 1024 < padded <= 2048 (DPOSER_SMALL64_MIN / _MAX)
#   time branch    the same thresholds on embed_dim channels, whatever the hidden width; 256x256 only for swish
#   post_dense/dx  64x32 up to 16384 padded samples (DPOSER_FINAL_SMALL_MAX), 64x128 above
#   wgrad H x H    128x128 split-K tiles, 256x256 from 32768
#   B: (padded, GN [bf16, H 1024, swish], GN [fp32 / bf16x3, H 1024, swish], GN [H 512 / 2048, or elu], time [swish], time [elu], final, wgrad)
DEFAULT = {
    1:     (64,    SMALL,   SMALL, SMALL, SMALL, SMALL, FINAL_S, MID),
    64:    (64,    SMALL,   SMALL, SMALL, SMALL, SMALL, FINAL_S, MID),
    65:    (128,   SMALL,   SMALL, SMALL, SMALL, SMALL, FINAL_S, MID),
    200:   (256,   SMALL,   SMALL, SMALL, SMALL, SMALL, FINAL_S, MID),
    512:   (512,   SMALL,   SMALL, SMALL, SMALL, SMALL, FINAL_S, MID),
    513:   (768,   SMALL,   SMALL, SMALL, SMALL, SMALL, FINAL_S, MID),
    1024:  (1024,  SMALL,   SMALL, SMALL, SMALL, SMALL, FINAL_S, MID),
    1025:  (1280,  SMALL64, SMALL, SMALL, SMALL, SMALL, FINAL_S, MID),
    2048:  (2048,  SMALL64, SMALL, SMALL, SMALL, SMALL, FINAL_S, MID),
    2049:  (2304,  MID,     MID,   MID,   MID,   MID,   FINAL_S, MID),
    2304:  (2304,  MID,     MID,   MID,   MID,   MID,   FINAL_S, MID),
    4096:  (4096,  MID,     MID,   MID,   MID,   MID,   FINAL_S, MID),
    4097:  (4352,  MID,     MID,   MID,   MID,   MID,   FINAL_S, MID),
    8192:  (8192,  MID,     MID,   MID,   MID,   MID,   FINAL_S, MID),
    16384: (16384, BIG,     BIG,   MID,   BIG,   MID,   FINAL_S, MID),
    16385: (16640, BIG,     BIG,   MID,   BIG,   MID,   FINAL,   MID),
    32768: (32768, BIG,     BIG,   MID,   BIG,   MID,   FINAL,   BIG),
    32769: (33024, BIG,     BIG,   MID,   BIG,   MID,   FINAL,   BIG),
    65536: (65536, BIG,     BIG,   MID,   BIG,   MID,   FINAL,   BIG),
}
# Launch forms:
#   weight gradients   one lane launch for all 256x256 tiles: the shipped widths (hidden 1024, embed 512) on sample-major operands (bf16, bf16x3);
#                      with bucket events (data parallel) bf16 takes two lane groups, bf16x3 the split-K launches; everything else split-K
#   time-branch dgrad  bf16x3: one GEMM per layer + reduce at every size; bf16: up to 2048 padded samples (DPOSER_SILU_SPLIT_MAX); fp32: one launch
#   second stream      split-K weight gradients between 8192 and 16384 padded samples
SIDE_STREAM_PADDED = (8192, 16384)


def expected_default(prec, H, act, B, events):
    padded, gn_bf16, gn_f32, gn_other, time_swish, time_elu, final, wgrad = DEFAULT[B]
    gn = gn_other if (H != 1024 or act != "swish") else (gn_bf16 if prec == "bf16" else gn_f32)
    lanes = H == 1024 and prec != "fp32"
    if lanes and not events:
        form, groups = SP.ONE_LAUNCH, 0
    elif lanes and events and prec == "bf16":
        form, groups = SP.LANE_GROUPS, 2
    else:
        form, groups = SP.SPLIT_K, 0
    split = 1 if prec == "bf16x3" else (1 if prec == "bf16" and padded <= 2048 else 0)
    side = 1 if form == SP.SPLIT_K and padded in SIDE_STREAM_PADDED else 0
    return SP.Plan(padded, gn, gn, time_swish if act == "swish" else time_elu, final, wgrad, form, groups, split, side)


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(prec="bf16", H=1024, act="swish", **kw):
        key = (prec, H, act, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = SP.make_handle(H, prec, act, **kw)
        return made[key]

    yield get
    for h in made.values():
        _C.lib().dposer_scorefc_destroy(h)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("H,act", [(512, "swish"), (1024, "swish"), (1024, "elu"), (2048, "swish")])      # (elu / relu / lrelu exist at hidden 1024 only)
def test_default_policy_is_the_documented_table(prec, H, act, handles, tuning_env):
    tuning_env()
    h = handles(prec, H, act)
    for B in BATCHES:
        for events in (False, True):
            assert SP.plan(h, B, events) == expected_default(prec, H, act, B, events), (prec, H, act, B, events)


def test_plan_refuses_bad_arguments_and_touches_no_gpu(handles):
    import ctypes as C
    lib = _C.lib()
    out = (C.c_int32 * 10)()
    assert lib.dposer_scorefc_plan(None, 8, 0, out) < 0 and b"NULL" in lib.dposer_last_error()
    assert lib.dposer_scorefc_plan(handles(), 8, 0, None) < 0 and b"NULL" in lib.dposer_last_error()
    assert lib.dposer_scorefc_plan(handles(), 0, 0, out) < 0 and b"batch" in lib.dposer_last_error()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dposer_hip.h")).read()
    assert "int dposer_scorefc_plan(dposer_scorefc_t h, int64_t batch, int32_t with_bucket_events, int32_t plan[10]);" in hdr
    assert lib.dposer_abi_version() == 1


# ------------------------------------------------------------------------------------------------
# forced policies of the GPU tests
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("B,padded", [(200, 256), (513, 768)])
def test_policy_big_puts_256x256_on_small_batches(prec, B, padded, handles, tuning_env):
    tuning_env(**SP.POLICY_BIG)
    for D in (63, 126):
        h = handles(prec, D=D)
        pl = SP.plan(h, B)
        assert pl[:6] == (padded, BIG, BIG, BIG, FINAL, BIG), pl
        assert pl.wgrad_form == (SP.SPLIT_K if prec == "fp32" else SP.ONE_LAUNCH) and pl.side_stream == 0
        assert pl.time_split == (1 if prec == "bf16x3" else 0)         # (256x256 has no k-split form: one launch outside bf16x3)
        tuning_env(DPOSER_WGRAD_BATCHED="0")
        assert SP.plan(h, B)[:8] == (padded, BIG, BIG, BIG, FINAL, BIG, SP.SPLIT_K, 0)
        tuning_env(DPOSER_WGRAD_BATCHED=None)
    pe = SP.plan(handles(prec), B, events=True)                          # the bucketed backward: lane groups in bf16
    assert (pe.wgrad_form, pe.groups) == ((SP.LANE_GROUPS, 2) if prec == "bf16" else (SP.SPLIT_K, 0))
    assert pe[:6] == (padded, BIG, BIG, BIG, FINAL, BIG)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("B,padded", [(65, 128), (200, 256), (513, 768)])
def test_policy_mid_puts_128x128_on_small_batches(prec, B, padded, handles, tuning_env):
    tuning_env(**SP.POLICY_MID)
    for D in (63, 126):
        h = handles(prec, D=D)
        pl = SP.plan(h, B)
        assert pl[:6] == (padded, MID, MID, MID, FINAL, MID), pl
        assert pl.wgrad_form == (SP.SPLIT_K if prec == "fp32" else SP.ONE_LAUNCH) and pl.side_stream == 0
        assert pl.time_split == (0 if prec == "fp32" else 1)
        tuning_env(DPOSER_WGRAD_BATCHED="0")
        assert SP.plan(h, B)[:8] == (padded, MID, MID, MID, FINAL, MID, SP.SPLIT_K, 0)
        tuning_env(DPOSER_WGRAD_BATCHED=None, DPOSER_SILU_SPLIT_MAX="0")
        assert SP.plan(h, B).time_split == (1 if prec == "bf16x3" else 0)
        tuning_env(DPOSER_SILU_SPLIT_MAX=None)
    pe = SP.plan(handles(prec), B, events=True)
    assert (pe.wgrad_form, pe.groups) == ((SP.LANE_GROUPS, 2) if prec == "bf16" else (SP.SPLIT_K, 0))


@pytest.mark.parametrize("prec", PRECISIONS)
def test_policies_on_the_bf16_faithful_cases(prec, handles, tuning_env):
    """tests/test_gpu_bf16_faithful.py: ``fwd_b200`` / ``drop*_b200`` (one block) and ``wgrad_b512`` under BIG and MID."""
    h = handles(prec, n_blocks=1)
    for name, tile in (("BIG", BIG), ("MID", MID)):
        SP.force(tuning_env, name)
        assert SP.plan(h, 200)[:5] == (256, tile, tile, tile, FINAL)
        assert SP.plan(h, 512)[:6] == (512, tile, tile, tile, FINAL, tile)
        tuning_env(DPOSER_WGRAD_BATCHED="0")
        assert SP.plan(h, 512)[:8] == (512, tile, tile, tile, FINAL, tile, SP.SPLIT_K, 0)
        tuning_env(DPOSER_WGRAD_BATCHED=None)


def test_forced_policies_of_the_existing_bf16_faithful_cases(handles, tuning_env):
    h = handles("bf16", n_blocks=1)
    tuning_env(DPOSER_BIG_MIN_BATCH="2304")                              # fwd_b2304: 256x256
    assert SP.plan(h, 2304)[:2] == (2304, BIG)
    tuning_env(DPOSER_BIG_MIN_BATCH=None, DPOSER_FINAL_SMALL_MAX="0")     # fwd_b1100: post_dense on 64x128 behind the eight-wave GroupNorm tiling
    assert SP.plan(h, 1100)[:5] == (1280, SMALL64, SMALL64, SMALL, FINAL)
    tuning_env(DPOSER_FINAL_SMALL_MAX=None, DPOSER_WGRAD_BATCHED="0", DPOSER_WGRAD_BIG="1", DPOSER_GNBWD_BIG="1")      # wgrad_b2304
    pl = SP.plan(h, 2304)
    assert (pl.padded, pl.gn, pl.gn_bwd, pl.wgrad, pl.wgrad_form, pl.time_split) == (2304, MID, BIG, BIG, SP.SPLIT_K, 0)
    tuning_env(DPOSER_WGRAD_BATCHED=None, DPOSER_WGRAD_BIG=None, DPOSER_GNBWD_BIG=None, DPOSER_WGRAD_TR="0")            # wgrad_b512_tr0
    pl = SP.plan(h, 512)
    assert (pl.gn, pl.wgrad_form, pl.time_split) == (SMALL, SP.SPLIT_K, 0)
    tuning_env(DPOSER_WGRAD_TR=None)
    pl = SP.plan(h, 512)                                                 # wgrad_b512: the defaults
    assert (pl.gn, pl.wgrad_form, pl.time_split) == (SMALL, SP.ONE_LAUNCH, 1)


TILING_ENVS = [      # the first two environments of test_gpu_score.py::test_alternative_tilings_and_streams_keep_parity
    ({"DPOSER_GNBWD_BIG": "1", "DPOSER_WGRAD_BIG": "1", "DPOSER_BIG_MIN_BATCH": "256", "DPOSER_WGRAD_BATCHED": "0"}, BIG),
    ({"DPOSER_GNBWD_BIG": "0", "DPOSER_WGRAD_BIG": "0", "DPOSER_WGRAD_STREAM": "0", "DPOSER_WGRAD_BATCHED": "0"}, MID),
]


@pytest.mark.parametrize("env,tile", TILING_ENVS)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_alternative_tiling_environments_with_and_without_the_small_tile_switch(env, tile, prec, handles, tuning_env):
    """Teeth: without DPOSER_SMALL_TILE_MAX=0 the two environments leave B = 1000 on 128x32 (only the split-K weight gradients obey
    them) -- what the child-process test ran from the day that switch arrived.  With it (and DPOSER_FINAL_SMALL_MAX=0) they force
    what they say."""
    h = handles(prec)
    tuning_env(**env)
    pl = SP.plan(h, 1000)
    assert (pl.padded, pl.gn, pl.gn_bwd, pl.time, pl.final) == (1024, SMALL, SMALL, SMALL, FINAL_S)
    assert (pl.wgrad, pl.wgrad_form) == (tile, SP.SPLIT_K)
    tuning_env(DPOSER_SMALL_TILE_MAX="0", DPOSER_FINAL_SMALL_MAX="0")
    assert SP.plan(h, 1000)[:8] == (1024, tile, tile, tile, FINAL, tile, SP.SPLIT_K, 0)
    assert SP.plan(h, 65)[:5] == (128, MID, MID, MID, FINAL)            # 128 padded samples cannot hold a 256-row tile


@pytest.mark.parametrize("prec", PRECISIONS)
def test_small_tile_switch_alone_on_the_other_widths_and_activations(prec, handles, tuning_env):
    """test_other_model_configurations_vs_oracle (hidden 512 / 2048) and test_other_activations_vs_reference_golden (elu at 384 samples)
    under DPOSER_SMALL_TILE_MAX=0: 128x128 where 128 divides the padded batch, 128x32 where it does not."""
    tuning_env(DPOSER_SMALL_TILE_MAX="0")
    for H in (512, 2048):
        h = handles(prec, H)
        assert SP.plan(h, 200)[:4] == (256, MID, MID, MID)
        assert SP.plan(h, 150)[:4] == (192, SMALL, SMALL, SMALL)
    assert SP.plan(handles(prec, 1024, "elu"), 384)[:4] == (384, MID, MID, MID)
    tuning_env(DPOSER_SMALL_TILE_MAX=None)
    assert SP.plan(handles(prec, 512), 200)[:4] == (256, SMALL, SMALL, SMALL)
    assert SP.plan(handles(prec, 1024, "elu"), 384)[:4] == (384, SMALL, SMALL, SMALL)
