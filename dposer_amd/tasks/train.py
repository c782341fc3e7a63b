"""The training run of run/train.py:96-410 -- model / EMA / optimizer / SDE / sampler / likelihood set-up, the step loop, logging,
checkpoints, resume, periodic validation -- without its CLI / absl / tensorboard shell.

What differs from the reference, on purpose:
  * the step is fed by ``dataset.feed.DeviceFeed`` (one HIP gather per mini-batch from a dataset resident in HBM) instead of a DataLoader
    over single poses plus a host-to-device copy per step (train.py:70-93, 247-248); the feed position follows from ``step`` alone, so a
    resumed run -- also from a checkpoint the reference wrote -- continues on the rows the uninterrupted run would have seen;
  * every loss key is accumulated on the device and read back once per ``log_freq`` steps, not ``.item()`` per key per step (train.py:254);
  * exceptions propagate (train.py:243, 406-407 print and swallow them), and a non-finite loss at a log point raises, naming the step;
  * under ``distributed.dp_active()`` every rank feeds its own shard of one global batch, rank 0 validates and writes, and every collective
    (the optimizer's ``gather_state`` before a checkpoint, the barrier behind validation) is entered by every rank.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import distributed as ddp
from ..algorithms.advanced import likelihood, losses, sampling, sde_lib
from ..algorithms.advanced.model import ScoreModelFC, TimeMLPs
from ..algorithms.ema import ExponentialMovingAverage
from ..dataset.AMASS import N_POSES, Evaler
from ..dataset.feed import DeviceFeed
from ..utils.metric import average_pairwise_distance, generation_fidelity
from ..utils.misc import create_mask

# the canvas and camera of the validation renders (train.py:46-48)
BG_SHAPE = (512, 384, 3)
FOCAL = [1500, 1500]
PRINCPT = [200, 192]
HYPO_NUM = 5                  # completions per test pose (train.py:286)
CHECKPOINT_KEYS = ("epoch", "model_state_dict", "optimizer_state_dict", "ema", "step")     # train.py:395-401


class _Task:
    """What the sampler reads of the reference's ``args`` (sampling.py:416: ``args.task``)."""

    def __init__(self, task):
        self.task = task


def build_model(config):
    """train.py:152-172."""
    pose_dim = 3 if config.data.rot_rep == "axis" else 6
    if config.model.type == "ScoreModelFC":
        return ScoreModelFC(config, n_poses=N_POSES, pose_dim=pose_dim, hidden_dim=config.model.HIDDEN_DIM, embed_dim=config.model.EMBED_DIM,
                            n_blocks=config.model.N_BLOCKS)
    if config.model.type == "TimeMLPs":
        return TimeMLPs(config, n_poses=N_POSES, pose_dim=pose_dim, hidden_dim=config.model.HIDDEN_DIM, n_blocks=config.model.N_BLOCKS)
    raise NotImplementedError("unsupported model")


def build_sde(config):
    """(sde, sampling_eps) of train.py:199-212."""
    name = config.training.sde.lower()
    if name == "vpsde":
        return sde_lib.VPSDE(beta_min=config.model.beta_min, beta_max=config.model.beta_max, N=config.model.num_scales), 1e-3
    if name == "subvpsde":
        return sde_lib.subVPSDE(beta_min=config.model.beta_min, beta_max=config.model.beta_max, N=config.model.num_scales), 1e-3
    if name == "vesde":
        return sde_lib.VESDE(sigma_min=config.model.sigma_min, sigma_max=config.model.sigma_max, N=config.model.num_scales), 1e-5
    raise NotImplementedError(f"SDE {config.training.sde} unknown.")


def _to_axis(config, x):
    if config.data.rot_rep == "rot6d":
        from ..utils.transforms import rot6d_to_axis_angle
        return rot6d_to_axis_angle(x.reshape(-1, 6)).reshape(*x.shape[:-1], N_POSES * 3)
    return x


def validate(state, sde, config, test_poses, body_model, denormalize, out_dir=None, *, render=False, log=None, device=None,
             fused_eval=False, fidelity_k=0):
    """The validation block of train.py:263-372 under the EMA weights: per test batch of ``config.eval.batch_size`` poses the bpd
    (likelihood ODE, rtol = atol = eps = 1e-4), five sampler completions of the left leg scored by ``Evaler.multi_eval_bodys`` and one
    generation; then APD over the first 22 joints of the first 50 samples and ``last_samples.npz`` (``pose_trajs [10, 5, D_axis]``,
    ``pose_samples [1, 50, D_axis]``) in ``out_dir``.  ``render=True`` adds the OBJ / image files of :338-362.  The model's parameters
    are restored and it is left in train mode.  ``fused_eval`` scores the completions with ``Evaler.multi_eval_bodys(fused=True)``.  Returns ``{'bpd', 'mpvpe_all', 'mpjpe_body', 'APD'}`` as floats.
    ``fidelity_k > 0`` adds the entries of ``utils.metric.generation_fidelity`` (``dNN``, ``precision``, ``recall``, ``density``,
    ``coverage`` at that k, and its ``APD`` as ``APD_all``), computed from ALL generated samples -- not the 50 kept for the dump -- against
    the first 22 joints of the test poses the batches covered."""
    model, ema = state["model"], state["ema"]
    device = torch.device(device) if device is not None else next(model.parameters()).device
    log = log or (lambda msg: None)
    bs = int(config.eval.batch_size)
    test_poses = test_poses.to(device)
    n_batches = test_poses.shape[0] // bs                                                  # drop_last (train.py:86-91)
    if n_batches < 1:
        raise ValueError(f"{test_poses.shape[0]} test poses do not fill one evaluation batch of {bs}")
    _, sampling_eps = build_sde(config)
    sampling_fn = sampling.get_sampling_fn(config, sde, (bs, test_poses.shape[1]), lambda x: x, sampling_eps, device=device)
    likelihood_fn = likelihood.get_likelihood_fn(sde, lambda x: x, rtol=1e-4, atol=1e-4, eps=1e-4)
    evaler = Evaler(body_model=body_model, part="left_leg")
    metrics = {"bpd": [], "mpvpe_all": [], "mpjpe_body": []}
    all_results, trajs = [], None
    model.eval()
    try:
        for b in range(n_batches):
            poses = test_poses[b * bs:(b + 1) * bs].contiguous()
            ema.store(model.parameters())
            ema.copy_to(model.parameters())
            try:
                bpd, _, nfe = likelihood_fn(model, poses)                                  # task 1: bpd
                metrics["bpd"].append(bpd.mean())
                with torch.no_grad():
                    mask, observation = create_mask(poses, part="left_leg")                # task 2: completion
                    hypos = torch.stack([sampling_fn(model, observation=observation, mask=mask, args=_Task("completion"), traj_stride=0)[1]
                                         for _ in range(HYPO_NUM)], dim=1)
                    preds = _to_axis(config, denormalize(hypos))
                    gts = _to_axis(config, denormalize(poses))
                    res = evaler.multi_eval_bodys(preds, gts, as_tensors=True, fused=fused_eval)
                    metrics["mpvpe_all"].append(res["mpvpe_all"].mean())
                    metrics["mpjpe_body"].append(res["mpjpe_body"].mean())
                    trajs, samples = sampling_fn(model, observation=None)                  # task 3: generation, [t, b, D], [b, D]
                    all_results.append(samples)
            finally:
                ema.restore(model.parameters())
            log(f"validate batch {b + 1}/{n_batches}: bpd {float(metrics['bpd'][-1]):.6f} (nfe {nfe}), "
                f"mpvpe_all {float(metrics['mpvpe_all'][-1]):.4f}, mpjpe_body {float(metrics['mpjpe_body'][-1]):.4f}")
        with torch.no_grad():
            trajs = trajs[::max(sde.N // 10, 1), :5]                                       # [10 times, 5 samples, D]
            all_results = torch.cat(all_results, dim=0)
            fidelity = {}
            if fidelity_k > 0:
                to_joints = lambda x: body_model(pose_body=_to_axis(config, denormalize(x)).reshape(-1, N_POSES * 3)).Jtr[:, :22, :].contiguous()
                fid = generation_fidelity(to_joints(all_results), to_joints(test_poses[:n_batches * bs]), k=int(fidelity_k))
                fidelity = {("APD_all" if key == "APD" else key): float(v) for key, v in fid.items()}
            all_results = all_results[:50]
            trajs = _to_axis(config, denormalize(trajs)).reshape(-1, N_POSES * 3)
            all_results = _to_axis(config, denormalize(all_results)).reshape(-1, N_POSES * 3)
            joints = body_model(pose_body=all_results).Jtr[:, :22, :]
            apd = float(average_pairwise_distance(joints))
            if render:
                _render(body_model, trajs, all_results, out_dir)
    finally:
        model.train()
    out = {k: float(torch.stack(v).mean()) for k, v in metrics.items()}
    out["APD"] = apd
    out.update(fidelity)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        np.savez(os.path.join(out_dir, "last_samples.npz"), pose_trajs=trajs.cpu().numpy().reshape(10, 5, -1),
                 pose_samples=all_results.cpu().numpy().reshape(1, 50, -1))
    return out


def _render(body_model, trajs, samples, out_dir):
    """train.py:338-362: OBJ files and renders of the trajectory bodies (sample x time) and of the 50 generated bodies.  Images are PNG
    (the built-in writer) where the reference writes JPEG through cv2."""
    from ..body_model.visual import render_mesh, save_obj, write_image
    if out_dir is None:
        raise ValueError("render=True needs out_dir")
    obj_dir, render_dir = os.path.join(out_dir, "obj_results"), os.path.join(out_dir, "render_results")
    os.makedirs(obj_dir, exist_ok=True)
    os.makedirs(render_dir, exist_ok=True)
    bg = np.ones(BG_SHAPE) * 255
    cam = {"focal": FOCAL, "princpt": PRINCPT}

    def emit(mesh, faces, obj_name, img_name):
        save_obj(mesh, faces, os.path.join(obj_dir, obj_name))
        img = render_mesh(bg, mesh, faces, cam)
        write_image(os.path.join(render_dir, img_name), np.clip(np.rint(img), 0, 255).astype(np.uint8))

    body = body_model(pose_body=trajs)
    faces = body.f.cpu().numpy()
    meshes = body.v.detach().cpu().numpy().reshape(10, 5, -1, 3)
    for s in range(5):
        for t in range(10):
            emit(meshes[t, s], faces, f"sample{s + 1}_time{t + 1}.obj", f"render_sample{s + 1}_time{t + 1}.png")
    meshes = body_model(pose_body=samples).v.detach().cpu().numpy()
    for s in range(meshes.shape[0]):
        emit(meshes[s], faces, f"Rsample{s + 1}.obj", f"Rrender_sample{s + 1}.png")


def train(config, train_set, test_set, body_model, out_dir, *, n_iters=None, resume=None, seed=None, log=print, on_eval=None):
    """Run the training of run/train.py to ``n_iters`` steps (default ``config.training.n_iters``).

    ``train_set`` / ``test_set``: ``AMASSDataset``s, or anything with ``.poses`` ([N, D] fp32, already normalised) and ``.Denormalize``.
    ``body_model``: the ``BodyModel`` of the validation (and of the auxiliary loss).  ``resume``: a checkpoint file of this function or of
    the reference.  ``seed``: key of the feed's permutation (default ``config.seed``; every rank passes the same).  ``on_eval(step,
    metrics)`` is called after each validation on the rank that ran it.  Returns ``(state, history)`` with ``history`` a list of
    ``(step, {loss key: mean over the steps since the last log point})``."""
    device = torch.device("cuda", torch.cuda.current_device())
    rank0 = ddp.rank() == 0
    n_iters = int(config.training.n_iters if n_iters is None else n_iters)
    log_freq, eval_freq, save_freq = int(config.training.log_freq), int(config.training.eval_freq), int(config.training.save_freq)
    if rank0:
        os.makedirs(out_dir, exist_ok=True)
    denormalize = train_set.Denormalize if config.data.normalize else (lambda x: x)

    model = build_model(config).to(device)
    ema = ExponentialMovingAverage(model.parameters(), decay=config.model.ema_rate)
    optimizer = losses.get_optimizer(config, model.parameters())
    state = dict(optimizer=optimizer, model=model, ema=ema, step=0)
    if resume is not None:                                                                 # train.py:186-191
        ck = torch.load(resume, map_location=device, weights_only=False)
        model.load_state_dict(ck["model_state_dict"])
        optimizer.load_state_dict(ck["optimizer_state_dict"])
        ema.load_state_dict(ck["ema"])
        state["step"] = int(ck["step"])
        log(f"=> loaded checkpoint '{resume}' (step {state['step']}, epoch {ck.get('epoch')})")

    sde, _ = build_sde(config)
    if config.training.auxiliary_loss:                                                     # train.py:218-226
        kwargs = {"denormalize": denormalize, "body_model": body_model, "rot_rep": config.data.rot_rep,
                  "denoise_steps": config.training.denoise_steps}
    else:
        kwargs = {}
    train_step_fn = losses.get_step_fn(sde, train=True, optimize_fn=losses.optimization_manager(config),
                                       reduce_mean=config.training.reduce_mean, continuous=config.training.continuous,
                                       likelihood_weighting=config.training.likelihood_weighting,
                                       auxiliary_loss=config.training.auxiliary_loss, **kwargs)

    feed = DeviceFeed(train_set.poses, int(config.training.batch_size), seed=int(getattr(config, "seed", 0) or 0) if seed is None else seed,
                      device=device)
    log(f"total train samples: {feed.N}, test samples: {len(test_set.poses)}, {feed.steps_per_epoch} steps per epoch")

    history, acc, n_acc, best_apd = [], {}, 0, 0.0
    model.train()
    step = state["step"]
    while step < n_iters:
        loss_dict = train_step_fn(state, batch=feed.batch(step), condition=None, mask=None)
        for key, value in loss_dict.items():                                               # device-side sums: no host read per step
            v = value.detach().double().reshape(())
            if key in acc:
                acc[key] += v
            else:
                acc[key] = v.clone()
        n_acc += 1
        step = state["step"]

        if step % log_freq == 0:
            keys = list(acc)
            means = (torch.stack([acc[k] for k in keys]) / n_acc).cpu().tolist()           # the one read-back of the window
            bad = [k for k, m in zip(keys, means) if not np.isfinite(m)]
            if bad:
                raise FloatingPointError(f"non-finite {', '.join(bad)} in the {n_acc} steps up to step {step}")
            entry = dict(zip(keys, means))
            history.append((step, entry))
            log(f"Iter: [{step}/{n_iters}, {step / n_iters * 100:.2f}%][{(step - 1) % feed.steps_per_epoch + 1}/{feed.steps_per_epoch}],\t"
                + "".join(f"{k}: {m:.6f},\t" for k, m in entry.items()))
            acc, n_acc = {}, 0

        if step % eval_freq == 0:                                                          # train.py:263-390
            if rank0:
                with ddp.local_only():                                                     # one rank works: nothing in here may be a collective
                    metrics = validate(state, sde, config, test_set.poses, body_model, denormalize, out_dir,
                                       render=bool(config.training.render), log=log, device=device)
                log(f"step {step}: " + ", ".join(f"{k} {v:.6f}" for k, v in metrics.items()))
                if metrics["APD"] > best_apd:
                    best_apd = metrics["APD"]
                    log(f"saving best checkpoint, APD: {best_apd}")
                    torch.save({"model_state_dict": model.state_dict(), "epoch": feed.epoch_of(step) + 1, "ema": ema.state_dict(),
                                "step": state["step"]}, os.path.join(out_dir, "best_model.pth"))
                if on_eval is not None:
                    on_eval(step, metrics)
            ddp.barrier()

        if step % save_freq == 0:                                                          # train.py:393-403
            optimizer.gather_state()                                                       # a collective after ZeRO-1 steps: every rank
            if rank0:
                torch.save({"epoch": feed.epoch_of(step) + 1, "model_state_dict": model.state_dict(),
                            "optimizer_state_dict": optimizer.state_dict(), "ema": ema.state_dict(), "step": state["step"]},
                           os.path.join(out_dir, f"checkpoint-step{state['step']}.pth"))
                log(f"Save checkpoint to {out_dir}")
    return state, history
