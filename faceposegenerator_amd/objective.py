"""The training objective's forward pass — what the reference's fine-tuning loop computes per step (SURVEY.md §8f-4;
/root/reference/train_ID-Booth.py:996-1134 and the log record :1153-1172), evaluated under ``no_grad``: the validation losses of a
(LoRA) checkpoint on held-out identity images.  The backward pass is out of scope.

One ``step_losses`` call is one step of the reference on a batch ordered ``[instances; priors]`` as its ``collate_fn`` builds it:

  1. ``vae.encode(pixel_values).latent_dist.sample() * scaling_factor``      :1001-1002   HipEngine.vae_encode
  2. ``add_noise`` and the target (``noise`` or ``get_velocity``)            :1018, :1055 idb_diffuse_targets
  3. ``unet(noisy, timesteps, encoder_hidden_states)``                       :1040        HipEngine.unet_forward, per-sample timesteps
  4. ``F.mse_loss`` of each half, ``step(...).pred_original_sample``          :1072, :1081 idb_objective_mse_x0
  5. for ``which_loss`` "identity" / "triplet_prior", per instance sample: decode the predicted x0 to a float [0, 255] HWC image
     (latents_to_image_for_mtcnn :433-442, no uint8 quantisation), ``mtcnn.detect(img, landmarks=False)`` (:1085), the first box
     truncated toward zero and clipped with max / min (:1088-1090), crop + bilinear resize to 112x112 + normalisation
     (idb_crop_resize_bilinear_f32), ``arcface(x)``, then ``1 - cos`` (:1096-1098) or the triplet loss against the instance's and the
     prior's embedding (:1133) in idb_identity_losses, weighted by ``(1 - t / T) ** 2`` (:1100).

Two places where the reference cannot be followed literally:

  * Undetected face.  The reference leaves ``identity_loss`` at the previous step's value (unbound on the first step) and logs that.
    Here the term is left out of ``combined``, ``id`` is 0 and ``detected`` is False.  A box that is empty after clipping counts as
    undetected (the reference would slice an empty, or for a negative end a wrapped, image).
  * Several instance samples.  The reference only ever scores sample 0 of a batch with one instance (``timesteps[0]``,
    ``gt_arcface_embed[0]``, ``gt_arcface_embed[1]``).  With N > 1 every instance sample i is scored against ``identity_embed[i]`` and
    ``identity_embed[N + i]``; ``id`` is the mean over the detected instances and the term added to ``combined`` the mean of
    ``weight_i * id_i`` over them.  With N = 1 this is the reference's formula.

There is no CPU path: the kernels are HIP (csrc/idb_objective.hip), and a missing library raises."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L

WHICH_LOSS = ("", "identity", "triplet_prior")          # configs/config_train_SD21.py:76 losses_to_test
LOG_KEYS = ("Step Loss/Reconstruction", "Step Loss/Prior", "Step Loss/ID", "Step Loss/Combined")      # train_ID-Booth.py:1171-1172
FACE = 112


# ---- host policy (pure functions, no GPU) -------------------------------------------------------------------------------------------
def clip_box(box, size: int) -> Optional[Tuple[int, int, int, int]]:
    """``bbox = bboxs[0].astype(int)`` (truncation toward zero) and ``img[max(0, b[1]):min(b[3], S), max(0, b[0]):min(b[2], S)]``
    (train_ID-Booth.py:1088-1090) -> (y0, y1, x0, x1) with exclusive ends, or None when the clipped box is empty."""
    b = np.asarray(box, dtype=np.float64).reshape(-1)[:4].astype(int)
    y0, y1, x0, x1 = max(0, int(b[1])), min(int(b[3]), size), max(0, int(b[0])), min(int(b[2]), size)
    return (y0, y1, x0, x1) if y1 > y0 and x1 > x0 else None


def timestep_weight(t: int, num_train_timesteps: int, timestep_loss_weighting: bool = True) -> float:
    """``identity_noise_level_weight = (1 - timesteps[0] / num_train_timesteps) ** 2``, or 1 when the weighting is off (:1100-1101)."""
    return (1.0 - int(t) / num_train_timesteps) ** 2 if timestep_loss_weighting else 1.0


def combine(instance: float, prior: float, id_losses: Sequence[float], weights: Sequence[float], detected: Sequence[bool],
            prior_loss_weight: float = 1.0, which_loss: str = "") -> Dict[str, float]:
    """``loss = instance_loss + prior_loss_weight * prior_loss`` (:1076) ``+ weight * id_loss`` (:1103, :1134) -> ``id``, ``weight`` and
    ``combined``.  The identity term is the mean of ``weight_i * id_i`` over the detected instances and absent when none is detected
    (or ``which_loss`` is ""); ``id`` and ``weight`` are the means of ``id_i`` and ``weight_i`` over the same instances."""
    if which_loss not in WHICH_LOSS:
        raise ValueError(f"which_loss {which_loss!r}: one of {WHICH_LOSS}")
    sel = [i for i, d in enumerate(detected) if d] if which_loss else []
    out = {"id": 0.0, "weight": float(np.mean(list(weights))) if len(weights) else 1.0, "combined": instance + prior_loss_weight * prior}
    if sel:
        out["id"] = float(np.mean([id_losses[i] for i in sel]))
        out["weight"] = float(np.mean([weights[i] for i in sel]))
        out["combined"] += float(np.mean([weights[i] * id_losses[i] for i in sel]))
    return out


def draw_step_inputs(latent_shape: Sequence[int], num_train_timesteps: int, generator: Optional[torch.Generator] = None):
    """The three random draws of a step in the reference's order: the encoder's sample noise (``latent_dist.sample()`` :1001), then
    ``torch.randn_like(model_input)`` (:1007), then ``torch.randint(0, T, (bsz,))`` (:1010) -> (latent_noise, noise, timesteps int64).
    Drawn on the generator's device (the CPU without one)."""
    dev = generator.device if generator is not None else torch.device("cpu")
    shape = tuple(int(v) for v in latent_shape)
    latent_noise = torch.randn(shape, generator=generator, dtype=torch.float32, device=dev)
    noise = torch.randn(shape, generator=generator, dtype=torch.float32, device=dev)
    timesteps = torch.randint(0, num_train_timesteps, (shape[0],), generator=generator, device=dev)
    return latent_noise, noise, timesteps.long()


def load_images(images, resolution: int = 512) -> torch.Tensor:
    """The dataset's transform (train_ID-Booth.py:293-300): ``Resize(resolution, BILINEAR)`` of the short side on the PIL image (Pillow's
    own resize on the host, as the reference's data loader runs it), a centre crop (the reference's RandomCrop is the identity on its
    square 512 images), ``ToTensor`` and ``Normalize([0.5], [0.5])`` -> fp32 [n, 3, resolution, resolution] in [-1, 1].
    ``images``: file paths, PIL images or uint8 RGB arrays [H, W, 3]."""
    from PIL import Image
    out = []
    for im in images:
        if isinstance(im, str):
            with Image.open(im) as f:
                im = f.convert("RGB")
        elif not isinstance(im, Image.Image):
            im = Image.fromarray(np.asarray(im, dtype=np.uint8))
        im = im.convert("RGB")
        w, h = im.size
        if min(w, h) != resolution:                    # torchvision Resize(int): short side to `resolution`, the long one int(size * long / short)
            nw, nh = (resolution, int(resolution * h / w)) if w <= h else (int(resolution * w / h), resolution)
            im = im.resize((nw, nh), Image.BILINEAR)
            w, h = nw, nh
        top, left = int(round((h - resolution) / 2.0)), int(round((w - resolution) / 2.0))      # torchvision center_crop
        a = np.asarray(im, dtype=np.uint8)[top:top + resolution, left:left + resolution]
        out.append((torch.from_numpy(a.copy()).permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5)
    return torch.stack(out)


# ---- kernels ------------------------------------------------------------------------------------------------------------------------
def _st() -> int:
    return torch.cuda.current_stream().cuda_stream


def _f32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.to(device=dev, dtype=torch.float32).contiguous()


def diffuse_targets(x0: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor, alphas_cumprod: torch.Tensor, v_prediction: bool):
    """idb_diffuse_targets: x0, noise fp32 NCHW on the device, timesteps int32 [B], alphas_cumprod fp32 [T] -> (noisy, target)."""
    lib = L.load()
    B, C, h, w = x0.shape
    noisy, target = torch.empty_like(x0), torch.empty_like(x0)
    L.check(lib.idb_diffuse_targets(x0.data_ptr(), noise.data_ptr(), timesteps.data_ptr(), alphas_cumprod.data_ptr(), alphas_cumprod.numel(),
                                    int(v_prediction), B, C, h * w, noisy.data_ptr(), target.data_ptr(), _st()), "idb_diffuse_targets")
    return noisy, target


def mse_x0(pred: torch.Tensor, target: torch.Tensor, noisy: Optional[torch.Tensor], timesteps: torch.Tensor, alphas_cumprod: torch.Tensor,
           v_prediction: bool, pred_nhwc: bool = False, want_x0: bool = True):
    """idb_objective_mse_x0: pred NCHW [B,C,h,w], or with pred_nhwc [B*h*w, C]; target / noisy NCHW -> (sse double [B], x0_pred or None)."""
    lib = L.load()
    B, C, h, w = target.shape
    sse = torch.empty((B,), dtype=torch.float64, device=target.device)
    x0 = torch.empty_like(target) if want_x0 else None
    need = lib.idb_objective_workspace_bytes(B, C * h * w)
    ws = torch.empty((max(need, 8),), dtype=torch.uint8, device=target.device)
    L.check(lib.idb_objective_mse_x0(pred.data_ptr(), int(pred_nhwc), target.data_ptr(), None if noisy is None else noisy.data_ptr(),
                                     timesteps.data_ptr(), alphas_cumprod.data_ptr(), alphas_cumprod.numel(), int(v_prediction), B, C, h * w,
                                     sse.data_ptr(), None if x0 is None else x0.data_ptr(), ws.data_ptr(), need, _st()), "idb_objective_mse_x0")
    return sse, x0


def crop_resize_bilinear(images: torch.Tensor, boxes: np.ndarray, oh: int = FACE, ow: int = FACE) -> torch.Tensor:
    """idb_crop_resize_bilinear_f32: float NHWC [B,H,W,C] in [0, 255], boxes int32 [n][5] = image, y0, y1, x0, x1 -> fp32 [n,C,oh,ow]."""
    lib = L.load()
    B, H, W, C = images.shape
    boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 5)
    n = boxes.shape[0]
    bx = torch.from_numpy(boxes).to(images.device)
    out = torch.empty((n, C, oh, ow), dtype=torch.float32, device=images.device)
    L.check(lib.idb_crop_resize_bilinear_f32(images.data_ptr(), B, H, W, C, bx.data_ptr(), n, out.data_ptr(), oh, ow, _st()),
            "idb_crop_resize_bilinear_f32")
    return out


def identity_losses(feat: torch.Tensor, pos: torch.Tensor, neg: Optional[torch.Tensor] = None):
    """idb_identity_losses: fp32 [n,d] each -> (cos, identity, triplet or None), fp32 [n]."""
    lib = L.load()
    n, d = feat.shape
    cos = torch.empty((n,), dtype=torch.float32, device=feat.device)
    ident = torch.empty_like(cos)
    trip = torch.empty_like(cos) if neg is not None else None
    L.check(lib.idb_identity_losses(feat.data_ptr(), pos.data_ptr(), None if neg is None else neg.data_ptr(), n, d, cos.data_ptr(),
                                    ident.data_ptr(), None if trip is None else trip.data_ptr(), _st()), "idb_identity_losses")
    return cos, ident, trip


# ---- the objective ------------------------------------------------------------------------------------------------------------------
class TrainingObjective:
    """``pipe``: a StableDiffusionPipeline on the device with VAE encoder weights; ``arcface`` / ``mtcnn``: the ArcFace and MTCNN
    objects (only needed for ``which_loss`` "identity" / "triplet_prior").  ``with_prior_preservation=False`` takes batches of
    instances only (:1136-1138: the reference then computes no prior and no identity term)."""

    def __init__(self, pipe, arcface=None, mtcnn=None, prior_loss_weight: float = 1.0, which_loss: str = "",
                 timestep_loss_weighting: bool = True, with_prior_preservation: bool = True):
        if which_loss not in WHICH_LOSS:
            raise ValueError(f"which_loss {which_loss!r}: one of {WHICH_LOSS}")
        if which_loss and not with_prior_preservation:
            raise ValueError("the reference computes the identity terms only under prior preservation (train_ID-Booth.py:1066-1135)")
        if which_loss and arcface is None:
            raise ValueError(f"which_loss {which_loss!r} needs an ArcFace model")
        self.pipe, self.arcface, self.mtcnn = pipe, arcface, mtcnn
        self.prior_loss_weight, self.which_loss = float(prior_loss_weight), which_loss
        self.timestep_loss_weighting, self.with_prior_preservation = bool(timestep_loss_weighting), bool(with_prior_preservation)
        self._ac = None

    def _engine(self):
        eng = self.pipe._engine()
        if not getattr(eng, "has_vae_encoder", False):
            sd = self.pipe.vae_encoder_state_dict()
            if sd is None:
                raise FileNotFoundError("this pipeline was built without VAE encoder weights")
            eng.pack_vae_encoder(sd)
        if self._ac is None or self._ac.device != eng.device:
            self._ac = _f32(self.pipe.scheduler.alphas_cumprod, eng.device)
        return eng

    def float_images(self, latents: torch.Tensor) -> torch.Tensor:
        """latents_to_image_for_mtcnn (:433-442) for a batch: scaled latents -> float NHWC [n,H,W,3] in [0, 255], never quantised."""
        img01, _ = self.pipe._engine().decode_images(latents, chunk=self.pipe.vae_chunk, want_u8=False)
        return img01.mul_(255.0)

    @torch.no_grad()
    def step_losses(self, pixel_values, identity_embed, encoder_hidden_states, timesteps=None, noise=None, latent_noise=None,
                    generator: Optional[torch.Generator] = None, detector: Optional[Callable] = None, keep: bool = False) -> dict:
        """pixel_values [2N,3,S,S] in [-1, 1] (N instances, then N priors; [N,...] without prior preservation), identity_embed [2N,512],
        encoder_hidden_states [2N,L,D].  ``timesteps`` [2N], ``noise`` and ``latent_noise`` [2N,C,S/8,S/8] default to
        ``draw_step_inputs`` (the reference's draw order) from ``generator``; pass all three for a reproducible call.
        ``detector(images float [N,H,W,3] in [0,255])`` -> per image None or boxes [k,4] (x0, y0, x1, y1), the first one is used;
        the default is ``mtcnn.detect(images, landmarks=False)[0]``.

        Returns a dict of Python floats ``instance``, ``prior``, ``id``, ``weight``, ``combined``; per-instance lists ``detected``,
        ``bbox`` ((y0, y1, x0, x1) or None), ``id_losses``, ``weights``, ``cos``; ``timesteps`` (list) and ``pred_original_sample``
        [N,C,h,w] on the device.  With ``keep`` also ``latents``, ``model_pred``, ``target``, ``noisy`` (NCHW, all 2N samples),
        ``images`` (the decoded float images), ``faces`` (the 112x112 ArcFace inputs of the detected instances) and ``features``.  See the module docstring for the undetected-face and
        N > 1 rules."""
        eng = self._engine()
        dev = eng.device
        sched = self.pipe.scheduler
        T = int(sched.config.num_train_timesteps)
        vpred = sched.config.prediction_type == "v_prediction"
        if sched.config.prediction_type not in ("epsilon", "v_prediction"):
            raise ValueError(f"Unknown prediction type {sched.config.prediction_type}")
        x = _f32(pixel_values, dev)
        B, S = x.shape[0], x.shape[2]
        if x.ndim != 4 or x.shape[2] != x.shape[3]:
            raise ValueError("pixel_values must be [B,3,S,S]: the reference clips both box axes to img.shape[0] (:1089-1090)")
        if self.with_prior_preservation and B % 2:
            raise ValueError("prior preservation needs a batch of N instances followed by N priors")
        N = B // 2 if self.with_prior_preservation else B
        down = self.pipe.vae_scale_factor
        lshape = (B, self.pipe.vae_config.latent_channels, x.shape[2] // down, x.shape[3] // down)
        if timesteps is None or noise is None or latent_noise is None:
            d_ln, d_n, d_t = draw_step_inputs(lshape, T, generator)
            latent_noise = d_ln if latent_noise is None else latent_noise
            noise = d_n if noise is None else noise
            timesteps = d_t if timesteps is None else timesteps
        t_host = [int(v) for v in torch.as_tensor(timesteps).reshape(-1).tolist()]
        if len(t_host) != B or tuple(noise.shape) != lshape:
            raise ValueError(f"timesteps must have {B} entries and noise the shape {lshape}")
        if min(t_host) < 0 or max(t_host) >= T:
            raise ValueError(f"timesteps must lie in [0, {T})")
        ts = torch.tensor(t_host, dtype=torch.int32, device=dev)

        lat = eng.vae_encode(x, latent_noise, scale=self.pipe.vae_config.scaling_factor, chunk=self.pipe.vae_chunk)[0]
        noisy, target = diffuse_targets(lat, _f32(noise, dev), ts, self._ac, vpred)
        pred = eng.unet_forward(noisy, ts.float(), encoder_hidden_states, nhwc=True)       # [B*h*w, C], the engine's layout
        want_id = bool(self.which_loss)
        sse, x0 = mse_x0(pred, target, noisy, ts, self._ac, vpred, pred_nhwc=True, want_x0=want_id or keep)
        out: dict = {}
        if keep:
            out["model_pred"] = pred.view(B, lshape[2] * lshape[3], lshape[1]).permute(0, 2, 1).reshape(lshape).clone()
            out["target"], out["noisy"], out["latents"] = target, noisy, lat
        per = sse.cpu() / float(lshape[1] * lshape[2] * lshape[3])
        instance = float(per[:N].mean())
        prior = float(per[N:].mean()) if self.with_prior_preservation else 0.0

        weights = [timestep_weight(t_host[i], T, self.timestep_loss_weighting) for i in range(N)]
        detected, bbox, id_losses, cosv = [False] * N, [None] * N, [0.0] * N, [None] * N
        if want_id:
            images = self.float_images(x0[:N])
            if detector is None:
                if self.mtcnn is None:
                    raise ValueError(f"which_loss {self.which_loss!r} needs an MTCNN detector (or a `detector` callable)")
                detector = lambda im: self.mtcnn.detect(im, landmarks=False)[0]      # noqa: E731
            found = detector(images)
            for i in range(N):
                b = None if found is None else found[i]
                bbox[i] = None if b is None or np.size(b) == 0 else clip_box(np.asarray(b, dtype=np.float64).reshape(-1, 4)[0], S)
                detected[i] = bbox[i] is not None
            sel = [i for i in range(N) if detected[i]]
            if sel:
                faces = crop_resize_bilinear(images, np.array([[i, *bbox[i]] for i in sel], dtype=np.int32))
                feat = self.arcface(faces)
                emb = _f32(identity_embed, dev)
                idx = torch.tensor(sel, device=dev)
                pos = emb[idx].contiguous()
                neg = emb[idx + N].contiguous() if self.which_loss == "triplet_prior" else None
                cos, ident, trip = identity_losses(feat, pos, neg)
                loss, cos_host = (trip if neg is not None else ident).cpu().tolist(), cos.cpu().tolist()
                for k, i in enumerate(sel):
                    id_losses[i], cosv[i] = float(loss[k]), float(cos_host[k])
                if keep:
                    out["faces"], out["features"] = faces, feat
            if keep:
                out["images"] = images
        out.update(combine(instance, prior, id_losses, weights, detected, self.prior_loss_weight, self.which_loss))
        out.update(instance=instance, prior=prior, detected=detected, bbox=bbox, id_losses=id_losses, weights=weights, cos=cosv,
                   timesteps=t_host, pred_original_sample=None if x0 is None else x0[:N])
        return out


def validation_losses(objective: TrainingObjective, instance_images, class_images, instance_embeds, class_embeds, prompt_embeds,
                      n_draws: int = 8, seed: int = 0, resolution: Optional[int] = None, detector: Optional[Callable] = None) -> dict:
    """Mean step losses of a checkpoint over ``n_draws`` seeded draws of batch [1 instance; 1 prior].  Draw k takes instance image
    ``k % len(instance_images)`` and class image ``k % len(class_images)`` (the dataset's ``index % num_*_images``, :307, :329) with
    their embeddings; ``prompt_embeds`` [2,L,D] are the instance and the class prompt.  Images: tensors [n,3,S,S] in [-1, 1], or
    what ``load_images`` takes.  All randomness comes from one ``torch.Generator().manual_seed(seed)`` in the reference's order, so a
    second call returns the same record: the reference's log keys (means over the draws; ``Step Loss/ID`` over the draws with a
    detected face), ``detection_rate``, and the per-draw lists under ``draws``.  ``detector`` is handed to ``step_losses``."""
    def tens(v):
        if torch.is_tensor(v):
            return v
        return load_images(v, resolution or objective.pipe.unet_config.sample_size * objective.pipe.vae_scale_factor)

    inst, cls = tens(instance_images), (tens(class_images) if objective.with_prior_preservation else None)
    ie, ce = torch.as_tensor(instance_embeds).float(), (torch.as_tensor(class_embeds).float() if cls is not None else None)
    g = torch.Generator().manual_seed(int(seed))
    draws: Dict[str, List] = {k: [] for k in ("instance", "prior", "id", "weight", "combined", "detected", "timesteps")}
    for k in range(int(n_draws)):
        i = k % inst.shape[0]
        px, em = inst[i:i + 1], ie[i:i + 1]
        if cls is not None:
            j = k % cls.shape[0]
            px, em = torch.cat([px, cls[j:j + 1]]), torch.cat([em, ce[j:j + 1]])
        r = objective.step_losses(px, em, prompt_embeds[:px.shape[0]], generator=g, detector=detector)
        for key in ("instance", "prior", "id", "weight", "combined", "timesteps"):
            draws[key].append(r[key])
        draws["detected"].append(bool(r["detected"][0]))
    mean = lambda v: float(np.mean(v)) if len(v) else 0.0      # noqa: E731
    hit = [v for v, d in zip(draws["id"], draws["detected"]) if d]
    return {"Step Loss/Reconstruction": mean(draws["instance"]), "Step Loss/Prior": mean(draws["prior"]), "Step Loss/ID": mean(hit),
            "Step Loss/Combined": mean(draws["combined"]),
            "detection_rate": mean([float(d) for d in draws["detected"]]) if objective.which_loss else 0.0,
            "n_draws": int(n_draws), "seed": int(seed), "draws": draws}
