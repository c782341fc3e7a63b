"""tasks/train.py on the GPU: ``train()`` is the hand-written loop over ``get_step_fn``'s step fed by ``DeviceFeed`` -- bit for bit in
parameters, EMA shadows and Adam moments -- its log windows are the means of that loop's losses, a run resumed from its own checkpoint ends
where the uninterrupted run ends, validation runs at its steps, leaves the model untouched and writes its files, and a NaN row in the
dataset stops the run at the next log point.

Setting: the shipped ScoreModelFC (1024 / 512 / 2 blocks, dropout 0.1, in-kernel draws) in fp32, sub-VP SDE with 50 scales, 4096 z-scored
toy rows, batches of 64, the synthetic SMPL-X asset, evaluation batches of 50."""
import os

import numpy as np
import pytest
import torch

import feed_ref
from gpu_common import DEV
from helpers import load

pytestmark = pytest.mark.gpu

N, B, STEPS, INIT_SEED = 4096, 64, 12, 7


class ToySet:
    """.poses / .Denormalize of an AMASSDataset (z-score statistics of golden g10_normalizer, axis-angle)."""

    def __init__(self, n, seed):
        g = load("g10_normalizer")
        raw = g["toy_pose_samples"].astype(np.float32)
        idx = np.random.RandomState(seed).randint(0, raw.shape[0], size=n)
        self.mean = torch.tensor(g["stats/axis_normalize2/mean_poses"].astype(np.float32))
        self.std = torch.tensor(g["stats/axis_normalize2/std_poses"].astype(np.float32))
        self.poses = torch.tensor(((raw[idx] - self.mean.numpy()) / self.std.numpy()).astype(np.float32))

    def Denormalize(self, poses, shapes=None):
        return poses * self.std.to(poses.device) + self.mean.to(poses.device)


def _config(**training):
    from dposer_amd.configs import load_config
    cfg = load_config("configs.subvp.amass_scorefc_continuous.get_config")
    cfg.seed = 1234
    cfg.model["precision"] = "fp32"
    cfg.model.num_scales = 50
    cfg.optim.warmup = 2                                   # (the default 5000 leaves the first steps with a learning rate near zero)
    cfg.training.batch_size = B
    cfg.eval.batch_size = 50
    cfg.training.log_freq = cfg.training.eval_freq = cfg.training.save_freq = 10 ** 6
    for k, v in training.items():
        cfg.training[k] = v
    return cfg


def _body():
    from dposer_amd.body_model.body_model import BodyModel
    from dposer_amd.body_model.synthetic import make_synthetic_smplx_asset
    return BodyModel(make_synthetic_smplx_asset(seed=0)).to(DEV)


def _snapshot(state):
    opt = state["optimizer"]
    return dict(params=state["model"].flat_params().detach().clone(), shadows=[s.detach().clone() for s in state["ema"].shadow_params],
                m=opt._flat_m.clone(), v=opt._flat_v.clone(), step=state["step"], num_updates=state["ema"].num_updates)


def _same(a, b):
    assert a["step"] == b["step"] and a["num_updates"] == b["num_updates"]
    assert torch.equal(a["params"], b["params"])
    assert len(a["shadows"]) == len(b["shadows"]) and all(torch.equal(x, y) for x, y in zip(a["shadows"], b["shadows"]))
    assert torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"])


def _train(cfg, sets, out_dir, **kw):
    from dposer_amd.tasks.train import train
    torch.manual_seed(INIT_SEED)                           # train() builds its model itself: same initial weights as the hand loop
    lines = []
    state, history = train(cfg, sets[0], sets[1], kw.pop("body", None), str(out_dir), log=lines.append, **kw)
    return state, history, lines


@pytest.fixture(scope="module")
def sets():
    return ToySet(N, 4096), ToySet(50, 50)


@pytest.fixture(scope="module")
def hand(sets):
    """The reference of this file, computed once: 12 steps of get_step_fn's step called by hand on feed.batch(0 .. 11)."""
    from dposer_amd.algorithms.advanced import losses
    from dposer_amd.algorithms.ema import ExponentialMovingAverage
    from dposer_amd.dataset.feed import DeviceFeed
    from dposer_amd.tasks.train import build_model, build_sde
    cfg = _config()
    torch.manual_seed(INIT_SEED)
    model = build_model(cfg).to(DEV)
    state = dict(optimizer=losses.get_optimizer(cfg, model.parameters()), model=model,
                 ema=ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate), step=0)
    start = model.flat_params().detach().clone()
    fn = losses.get_step_fn(build_sde(cfg)[0], train=True, optimize_fn=losses.optimization_manager(cfg), reduce_mean=True, continuous=True,
                            likelihood_weighting=False, auxiliary_loss=False)
    feed = DeviceFeed(sets[0].poses, B, seed=cfg.seed, num_replicas=1, rank=0)
    model.train()
    step_losses = []
    for s in range(STEPS):
        batch = feed.batch(s)
        assert np.array_equal(feed.indices(s).cpu().numpy(), feed_ref.indices(s, N, B, cfg.seed))
        step_losses.append({k: float(v) for k, v in fn(state, batch).items()})
    snap = _snapshot(state)
    assert not torch.equal(snap["params"], start)          # the run moved the weights
    return snap, step_losses


@pytest.fixture(scope="module")
def full_run(sets, tmp_path_factory):
    """train() for 12 steps with log_freq 4 and save_freq 6 (shared by the loop, logging and resume cases)."""
    out = tmp_path_factory.mktemp("full")
    state, history, lines = _train(_config(log_freq=4, save_freq=6), sets, out, n_iters=STEPS)
    return _snapshot(state), history, lines, out


def test_train_equals_the_hand_written_loop(hand, full_run):
    _same(full_run[0], hand[0])                            # bit-equal: parameters, EMA shadows, Adam moments, counters


def test_log_windows_are_the_means_of_the_hand_loop_losses(hand, full_run):
    _, step_losses = hand
    _, history, lines, _ = full_run
    assert [s for s, _ in history] == [4, 8, 12]
    for s, entry in history:
        assert set(entry) == set(step_losses[0]) == {"step_loss", "score_loss"}
        for k, got in entry.items():
            want = float(np.mean([d[k] for d in step_losses[s - 4:s]]))
            print(f"log window ending at step {s}: {k} {got:.8f}, hand loop {want:.8f}")
            assert abs(got - want) <= 1e-6 * abs(want), (s, k)
    assert sum(line.startswith("Iter: [") for line in lines) == 3


def test_resume_continues_bit_for_bit(hand, full_run, sets, tmp_path):
    from dposer_amd.tasks.train import CHECKPOINT_KEYS
    _, _, _, out = full_run
    assert sorted(f for f in os.listdir(out) if f.endswith(".pth")) == ["checkpoint-step12.pth", "checkpoint-step6.pth"]
    ck = torch.load(out / "checkpoint-step6.pth", map_location="cpu", weights_only=False)
    assert set(ck) == set(CHECKPOINT_KEYS) == {"epoch", "model_state_dict", "optimizer_state_dict", "ema", "step"}
    assert ck["step"] == 6 and ck["epoch"] == 1            # 64 steps per epoch: step 6 lies in epoch 0, stored as epoch + 1
    torch.manual_seed(INIT_SEED + 1)                       # other initial weights: everything must come from the file
    from dposer_amd.tasks.train import train
    state, history = train(_config(log_freq=4, save_freq=6), sets[0], sets[1], None, str(tmp_path), n_iters=STEPS,
                           resume=str(out / "checkpoint-step6.pth"), log=lambda m: None)
    _same(_snapshot(state), full_run[0])
    _same(_snapshot(state), hand[0])
    assert [s for s, _ in history] == [8, 12] and os.path.exists(tmp_path / "checkpoint-step12.pth")


def test_validation_runs_at_its_steps_and_leaves_the_model_alone(sets, tmp_path):
    import dposer_amd.tasks.train as T
    body = _body()
    seen, calls = [], []
    real = T.validate

    def spy(state, *a, **kw):
        before = state["model"].flat_params().detach().clone()
        out = real(state, *a, **kw)
        calls.append((state["step"], torch.equal(before, state["model"].flat_params()), state["model"].training))
        return out

    T.validate = spy
    try:
        state, _, _ = _train(_config(eval_freq=6), sets, tmp_path, n_iters=STEPS, body=body, on_eval=lambda s, m: seen.append((s, m)))
    finally:
        T.validate = real
    assert calls == [(6, True, True), (12, True, True)]    # called at 6 and 12; parameters bit-equal and train mode afterwards
    assert [s for s, _ in seen] == [6, 12]
    for _, m in seen:
        assert set(m) == {"bpd", "mpvpe_all", "mpjpe_body", "APD"}
        print("validation metrics:", m)
        assert all(isinstance(v, float) and np.isfinite(v) for v in m.values())
    z = np.load(tmp_path / "last_samples.npz")
    assert z["pose_trajs"].shape == (10, 5, 63) and z["pose_samples"].shape == (1, 50, 63)
    best = torch.load(tmp_path / "best_model.pth", map_location="cpu", weights_only=False)
    assert set(best) == {"model_state_dict", "epoch", "ema", "step"} and best["step"] in (6, 12)


def test_a_nan_row_stops_the_run_at_the_next_log_point(sets, tmp_path):
    cfg = _config(log_freq=4)
    bad = ToySet(N, 4096)
    row = int(feed_ref.indices(1, N, B, cfg.seed)[3])      # a row of the second batch
    bad.poses[row] = float("nan")
    with pytest.raises(FloatingPointError, match="step 4"):
        _train(cfg, (bad, sets[1]), tmp_path, n_iters=STEPS)
    assert not any(f.endswith(".pth") for f in os.listdir(tmp_path))
