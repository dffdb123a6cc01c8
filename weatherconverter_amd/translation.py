"""Guided weather translation loop (reference ``translation.py:46-97``, ``sample_with_sgg``).

Per reverse step i (N = 500 over the T = 1000 schedule, lambda = 60):
    eps = UNet(xt, i)                                   HIP engine
    mu, sigma*z = scheduler.sample_prev_timestep(...)   HIP kernel (sigma is sigma_t * z, D5)
    sr_xt = SRGAN(xt)                                   PyTorch-ROCm, x4
    odd i: xt = apply_gsg(...)   even i: xt = apply_lcg(...)   (segmenter fwd+input-grad + HIP update)
    xt = mu + sigma                                     reference line 90 (D1: overwrites the guidance)

``mode='reference'`` keeps D1 (guidance computed, then discarded) — the reference's effective output;
``mode='applied'`` keeps the guided xt on guided steps.  D2 (``mu + None`` TypeError at i = 0) is not
reproduced: the last step returns ``mu`` as ``sample_ddpm`` does.  LCG runs only when ``use_lcg``
(the reference's LCG crashes, D3; see ``sgg.apply_lcg``).

``steps=`` walks a sub-sequence tau of [0, N) instead (``timestep_sequence`` with N in place of T), with
(mu, sigma*z) from ``scheduler.ddim_prev_timestep``; GSG runs where the position k of tau is odd and LCG
on even k, which at stride 1 is the parity of i above.

``translate_files`` drives the loop from files (``load_image`` for the frame, ``seg_model.datasets.label_for``
for its labelIds map) and scores the result with the segmenter the guidance used; ``python -m
weatherconverter_amd.translation`` is the reference's ``__main__`` (``translation.py:100-162``) with its
hard-coded paths as arguments.
"""
from typing import Optional

import torch

from .diffusion_model.dataloader import load_image  # noqa: F401  (translation.py:131-143: the input of sample_with_sgg)
from .sgg.sgg import apply_gsg, apply_lcg
from .srgan_model.models import inference as srgan_inference


class _Replay:
    """fn(x) captured into a HIP graph over a static input buffer: a call copies x in and replays
    (the per-kernel host launch cost of a B=1 UNet / SRGAN forward is most of its eager time).  The
    returned tensor is the graph's static output: consumed before the next call."""

    def __init__(self, fn, x: torch.Tensor):
        self.x = x.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):  # allocations and weight packing outside the capture
                self.y = fn(self.x)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.y = fn(self.x)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        self.x.copy_(x)
        self.graph.replay()
        return self.y


@torch.no_grad()
def sample_with_sgg(input_tensor: torch.Tensor, diff_model, diff_scheduler, seg_model, gt: torch.Tensor,
                    srgan_model, *, LAMBDA: float = 60.0, N: int = 500, mode: str = 'applied', use_lcg: bool = False,
                    t_start: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                    progress=None, return_latent: bool = False, graph: bool = True, steps: Optional[int] = None,
                    spacing: str = 'trailing', eta: float = 1.0, clip_x0: bool = False):
    """graph=True replays the UNet and SRGAN forwards from HIP graphs (same kernels, same results);
    the segmenter's autograd pass stays eager.  steps=: DDIM transitions over `steps` of the N timesteps
    (eta = 1: the respaced ancestral chain; the guidance scales with sigma, so eta = 0 is refused)."""
    if mode not in ('reference', 'applied'):
        raise ValueError("mode must be 'reference' or 'applied'")
    tau = None
    if steps is not None:
        from .diffusion_model.scheduler.linear_noise_scheduler import timestep_sequence
        tau = timestep_sequence(N, steps, spacing=spacing)
        if not eta > 0:
            raise ValueError('sample_with_sgg: the strided guided loop needs eta > 0 (sigma = 0 means no guidance)')
    dev = diff_scheduler.device
    x0 = input_tensor.to(dev, torch.float32)
    # forward process (translation.py:63-65): random t in [0, N), one noising of the input
    t = torch.randint(0, N, (x0.shape[0], )) if t_start is None else t_start
    nz = torch.randn_like(x0) if noise is None else noise.to(dev)
    xt = diff_scheduler.add_noise2(x0, nz, t.to(dev))
    ts = torch.arange(N, device=dev, dtype=torch.long)
    unet_run = sr_run = None
    if graph and xt.is_cuda:
        from .diffusion_model.sample_ddpm import _GraphStep
        unet_run = _GraphStep(diff_model, xt)
        sr_run = _Replay(lambda v: srgan_inference(srgan_model, v), xt)
    # the reference's loop visits every i of [0, N) as hop i -> i - 1 at position k = i
    hops = [(i, i - 1, i) for i in reversed(range(N))] if tau is None else \
        [(tau[k], tau[k - 1] if k > 0 else -1, k) for k in reversed(range(len(tau)))]
    for i, i_to, k in hops:
        eps = unet_run(xt, ts[i:i + 1]) if unet_run is not None else diff_model(xt, ts[i:i + 1])
        if tau is None:
            mu, sigma, _ = diff_scheduler.sample_prev_timestep(xt, eps, i)
        else:
            mu, sigma, _ = diff_scheduler.ddim_prev_timestep(xt, eps, i, i_to, eta=eta, clip_x0=clip_x0)
        if k == 0:
            xt = mu
            break
        sr_xt = sr_run(xt) if sr_run is not None else srgan_inference(srgan_model, xt)
        guided = None
        if k % 2 == 1:
            guided = apply_gsg(seg_model, mu, sigma, sr_xt, gt, LAMBDA)
        elif use_lcg:
            guided = apply_lcg(seg_model, mu, sigma, sr_xt, gt, LAMBDA, mode=mode)
        if mode == 'applied' and guided is not None:
            xt = guided.contiguous()
        else:
            xt = (mu + sigma).contiguous()  # translation.py:90
        if progress is not None:
            progress(i)
    sr_x0 = srgan_inference(srgan_model, xt)  # translation.py:95
    return (sr_x0, xt) if return_latent else sr_x0


def srgan_scale(srgan_model) -> int:
    """The generator's upscale factor: one x2 PixelShuffle block per ``upsampler`` entry."""
    return 2 ** len(srgan_model.upsampler)


def _num_classes(seg_model) -> int:
    return seg_model.classifier.classifier[-1].out_channels


def translate_files(image_path, label_path, diff_model, diff_scheduler, seg_model, srgan_model, *,
                    image_size: Optional[int] = None, **sample_kwargs) -> dict:
    """One guided translation from files.  The frame goes through ``load_image(image_path, image_size)``
    (``image_size`` defaults to the UNet's ``im_size``), the labelIds file through ``label_for`` at the SRGAN
    factor, so both show the same field of view; ``sample_with_sgg(**sample_kwargs)`` translates, and the
    segmenter the guidance used scores the output against the label.  Returns ``{'output': (1, 3, S, S) fp32,
    'pred': uint8 (1, S, S) prediction on the output, 'score': the StreamSegMetrics results dict}``; everything
    stays on the device until the score's counts are read."""
    from .seg_model.datasets import label_for
    from .seg_model.inference import predict
    from .seg_model.metrics import StreamSegMetrics
    if sample_kwargs.get('return_latent'):
        raise ValueError('translate_files returns the super-resolved output only')
    dev = diff_scheduler.device
    S = int(image_size if image_size is not None else diff_model.model_config.im_size)
    x = load_image(image_path, S, dev)
    gt = label_for(label_path, S, scale=srgan_scale(srgan_model), device=dev)
    output = sample_with_sgg(x, diff_model, diff_scheduler, seg_model, gt, srgan_model, **sample_kwargs)
    metrics = StreamSegMetrics(_num_classes(seg_model), dev)
    pred = predict(seg_model, output, metrics=metrics, gt=gt)
    return {'output': output, 'pred': pred, 'score': metrics.get_results()}


def main(argv=None) -> dict:
    """The reference's ``__main__`` with its paths as arguments: translate --image guided by --labels, write
    ``output.png`` and the colourised prediction ``pred_color.png`` under --out, print the score."""
    import argparse
    import os

    from .diffusion_model import sample_ddpm as ddpm
    from .seg_model import inference as seg_infer
    from .seg_model.datasets import decode_target
    from .seg_model.metrics import StreamSegMetrics
    from .srgan_model import models as srgan
    ap = argparse.ArgumentParser(prog='weatherconverter_amd.translation', description=main.__doc__)
    ap.add_argument('--image', required=True, help='the frame (RGB image file)')
    ap.add_argument('--labels', required=True, help='its Cityscapes labelIds PNG (mode L)')
    ap.add_argument('--diff-config', required=True, help="the diffusion model's config.yaml")
    ap.add_argument('--diff-ckpt', required=True)
    ap.add_argument('--seg-ckpt', required=True)
    ap.add_argument('--srgan-ckpt', required=True)
    ap.add_argument('--out', required=True, help='output directory')
    ap.add_argument('--steps', type=int, default=None, help='strided sampling over this many of the N timesteps')
    ap.add_argument('--mode', choices=('applied', 'reference'), default='applied')
    ap.add_argument('--N', type=int, default=500, help='timesteps of the guided loop (reference: 500)')
    ap.add_argument('--LAMBDA', type=float, default=60.0, help='guidance weight (reference: 60)')
    args = ap.parse_args(argv)
    config = ddpm.load_config(args.diff_config)
    diff_model = ddpm.load_model(args.diff_ckpt, config.model)
    diff_scheduler = ddpm.load_scheduler(config.diffusion)
    srgan_model = srgan.load_model(args.srgan_ckpt)
    seg_model = seg_infer.load_model(args.seg_ckpt)
    res = translate_files(args.image, args.labels, diff_model, diff_scheduler, seg_model, srgan_model,
                          image_size=config.model.im_size, steps=args.steps, mode=args.mode, N=args.N, LAMBDA=args.LAMBDA)
    os.makedirs(args.out, exist_ok=True)
    ddpm.save_png(res['output'][0].clamp(0, 1), os.path.join(args.out, 'output.png'))
    ddpm.save_png(decode_target(res['pred'])[0].permute(2, 0, 1), os.path.join(args.out, 'pred_color.png'))
    print(StreamSegMetrics.to_str(res['score']))
    return res


if __name__ == '__main__':
    main()
