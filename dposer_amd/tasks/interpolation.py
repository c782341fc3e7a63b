"""Latent pose interpolation -- library form of the ``interpolation`` task of the reference's run/demo.py:412-504.

In network coordinates: the caller normalises the anchor poses before and denormalises the results after (as with ``DPoserComp``);
rendering and video writing stay with the caller (``body_model.visual.render_meshes`` draws any number of frames in one call).

* ``encode``: anchor poses -> probability-flow ODE latents z through ``likelihood_fn`` (demo.py:432, the reference's route; device
  resident here);
* ``decode``: latents -> poses with the deterministic sampler (probability_flow = True, Euler-Maruyama predictor, corrector 'none',
  demo.py:437-450) -- ONE ``dposer_pf_sampler`` call for any number of latents;
* ``slerp_segments``: the slerped latents between consecutive anchors (demo.py:466, ``utils.misc.slerp_interpolation``);
* ``interpolate``: all three; the S x frames latents of every segment are decoded in one sampler call, where the reference makes one
  call per pair.
"""
import torch

from ..algorithms.advanced import likelihood, sampling
from ..utils.misc import slerp_interpolation


def encode(model, sde, x, *, rtol=1e-4, atol=1e-4, eps=1e-4, epsilon=None):
    """Poses [n, D] (network coordinates) -> their ODE latents z [n, D]: ``likelihood_fn(model, x)[1]`` with demo.py:121's tolerances.
    ``epsilon``: the Hutchinson probe (RK45's step control sees the divergence too); None draws it as the reference does."""
    fn = likelihood.get_likelihood_fn(sde, lambda v: v, rtol=rtol, atol=atol, eps=eps)
    was_training = model.training
    model.eval()
    try:
        _, z, _ = fn(model, x, epsilon=epsilon)
    finally:
        model.train(was_training)
    return z


DECODERS = ("pf", "dpm")


def decode(model, sde, z, eps=1e-5, *, continuous=True, seed=None, decoder="pf", decoder_kw=None):
    """Latents z [n, D] -> poses [n, D]: the probability-flow pc_sampler from z (demo.py:437-450), no trajectory kept.  Deterministic:
    the result does not depend on ``seed`` (it keys no draw on this path).  ``decoder="dpm"``: the same ODE solved by the few-step
    DPM-Solver++ sampler (``decoder_kw``: ``steps``, ``order``, ``skip_type``), also deterministic."""
    if decoder not in DECODERS:
        raise ValueError(f"unknown decoder {decoder!r}: expected one of {DECODERS}")
    z = z.reshape(-1, z.shape[-1])
    if decoder == "dpm":
        fn = sampling.get_dpm_sampler(sde, tuple(z.shape), lambda v: v, continuous=continuous, denoise=False, eps=eps, device=z.device,
                                      **(decoder_kw or {}))
        return fn(model, z=z.contiguous(), traj_stride=0, seed=seed)[1]
    fn = sampling.get_pc_sampler(sde, tuple(z.shape), sampling.EulerMaruyamaPredictor, sampling.NoneCorrector, lambda v: v, snr=0.16,
                                 n_steps=1, probability_flow=True, continuous=continuous, denoise=True, eps=eps, device=z.device)
    _, x = fn(model, z=z.contiguous(), traj_stride=0, seed=seed)
    return x


def slerp_segments(z, frames):
    """z [n, D] -> [n - 1, frames, D]: segment s is ``slerp_interpolation(z[s], z[s + 1], frames)`` (demo.py:466)."""
    if z.shape[0] < 2:
        return z.new_empty((0, frames, z.shape[-1]))
    return torch.stack([slerp_interpolation(z[s], z[s + 1], frames) for s in range(z.shape[0] - 1)])


def interpolate(model, sde, anchors, frames=60, eps=1e-5, *, continuous=True, encode_kw=None, decoder="pf", decoder_kw=None):
    """demo.py:412-504 without rendering: anchors [n, D] -> (anchor_z [n, D], reconstructions [n, D], frames [n - 1, frames, D]).
    The reconstructions decode the anchors' latents; the frames decode every segment's latents in one sampler call.
    ``decoder``: "pf" (the reference's 1000-step probability-flow sampler) or "dpm" (the few-step solver, ``decoder_kw``)."""
    anchor_z = encode(model, sde, anchors, **(encode_kw or {}))
    dec = dict(continuous=continuous, decoder=decoder, decoder_kw=decoder_kw)
    recon = decode(model, sde, anchor_z, eps, **dec)
    lat = slerp_segments(anchor_z, frames)
    S, D = lat.shape[0], lat.shape[-1]
    out = decode(model, sde, lat.reshape(S * frames, D), eps, **dec) if S else lat.clone()
    return anchor_z, recon, out.reshape(S, frames, D)
