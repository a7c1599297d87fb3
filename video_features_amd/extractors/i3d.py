"""I3D two-stream extractor: per 64-frame stack, 1024-d per stream.

Capability parity with the reference's ``ExtractI3D``
(reference models/i3d/extract_i3d.py): rgb+flow streams (``--streams``),
flow from RAFT / PWC / pre-computed flow JPG dirs (``--flow_type``),
stack/step 64 sliding windows needing stack+1 frames (flow is between
consecutive frames), short videos resampled to stack+1 frames by linspace,
smaller-edge resize to 256 before flow, center-crop 224 + [-1, 1] scaling
per stream, ``--show_pred`` Kinetics top-5.  Output keys: ``rgb`` /
``flow`` (+ fps, timestamps_ms).
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import transforms as T
from ..io.video import open_video, ImageDirReader
from ..models.i3d import I3D
from ..models.pwc import PWCNet
from ..models.raft import RAFT, InputPadder
from .base import BaseExtractor

DEFAULT_STACK_SIZE = 64
DEFAULT_STEP_SIZE = 64
RESIZE_SIDE = 256
CROP = 224


class ExtractI3D(BaseExtractor):
    output_feat_keys = ['rgb', 'flow']

    def __init__(self, args, external_call: bool = False):
        super().__init__(args, external_call)
        self.streams = self.cfg.streams or ['rgb', 'flow']
        self.stack_size = self.cfg.stack_size or DEFAULT_STACK_SIZE
        self.step_size = self.cfg.step_size or DEFAULT_STEP_SIZE
        self.flow_type = self.cfg.flow_type
        self.output_feat_keys = list(self.streams)

    def _maybe_load(self, model: torch.nn.Module, name: str) -> None:
        """``--weights_path`` for i3d is a DIRECTORY holding
        ``i3d_rgb.pt`` / ``i3d_flow.pt`` / ``raft.pth`` / ``pwc.pth``
        (the reference ships these as separate checkpoint files,
        reference extract_i3d.py:23-26); missing files stay random-init.
        ``module.``-prefixed (DataParallel-saved) keys are accepted."""
        wp = self.cfg.weights_path
        if not wp:
            return
        p = Path(wp)
        if not p.is_dir():
            # a plain file cannot name which of the (up to 4) stream models
            # it belongs to — loading it into all of them would crash on a
            # strict load into the wrong net mid-build
            raise ValueError(
                f'--weights_path for i3d must be a DIRECTORY containing '
                f'i3d_rgb.pt / i3d_flow.pt / raft.pth / pwc.pth, got file '
                f'{wp!r}')
        p = p / f'{name}.pt'
        if not p.exists():
            p = p.with_suffix('.pth')
        if not p.exists():
            return
        self.load_weights(model, str(p))

    def build_models(self, device: torch.device, dtype: torch.dtype):
        models = {}
        if 'rgb' in self.streams:
            rgb = I3D(modality='rgb')
            self._maybe_load(rgb, 'i3d_rgb')
            models['rgb'] = rgb.to(device, dtype).eval()
        if 'flow' in self.streams:
            flow = I3D(modality='flow')
            self._maybe_load(flow, 'i3d_flow')
            models['flow'] = flow.to(device, dtype).eval()
            if self.flow_type == 'raft':
                raft = RAFT(corr=self.cfg.raft_corr)
                self._maybe_load(raft, 'raft')
                raft = raft.to(device, dtype).eval()
                if device.type == 'cuda':
                    raft = raft.use_channels_last()
                models['flow_xtr'] = raft
            elif self.flow_type == 'pwc':
                pwc = PWCNet()
                self._maybe_load(pwc, 'pwc')
                models['flow_xtr'] = pwc.to(device, dtype).eval()
        return models

    # ------------------------------------------------------------ helpers
    def _read_raw_frames(self, video_path) -> (torch.Tensor, float):
        """Decode to uint8 (T, H, W, 3); the resize happens on the GPU in
        ``extract`` (uploading u8 is 12x lighter than resized floats, and
        CPU-side bicubic dominated the end-to-end profile)."""
        reader = open_video(video_path, self.tmp_path, self.extraction_fps)
        n = reader.frame_count
        need = self.stack_size + 1
        if n < need:
            # short video: resample to stack+1 frames by linspace
            # (reference extract_i3d.py:250-255)
            idxs = np.linspace(0, n - 1, need).round().astype(np.int64)
        else:
            idxs = np.arange(n)
        frames = torch.from_numpy(reader.read_frames(idxs))
        if torch.cuda.is_available():
            frames = frames.pin_memory()     # async-capable H2D upload
        return frames, reader.fps

    def _compute_flow(self, models, stacks: torch.Tensor) -> torch.Tensor:
        """(B, S+1, 3, H, W) frames → (B*S, 2, H, W) flow via RAFT or PWC
        (all frame pairs of the batch in one flow-net forward)."""
        im1 = stacks[:, :-1].reshape(-1, *stacks.shape[2:])
        im2 = stacks[:, 1:].reshape(-1, *stacks.shape[2:])
        if self.flow_type == 'raft':
            padder = InputPadder(im1.shape)
            p1, p2 = padder.pad(im1, im2)
            return padder.unpad(models['flow_xtr'](p1, p2, test_mode=True))
        return models['flow_xtr'](im1, im2)

    def _read_precomputed_flow(self, flow_dir: str, device, dtype,
                               count: int) -> torch.Tensor:
        """flow_x_*.jpg / flow_y_*.jpg dirs → (T, 2, H, W) float flow in
        [-20, 20] (reference extract_i3d.py:231-237, 266-278)."""
        xs = ImageDirReader(flow_dir, pattern=r'flow_x').read_frames(range(count))
        ys = ImageDirReader(flow_dir, pattern=r'flow_y').read_frames(range(count))
        fx = torch.from_numpy(xs[..., 0]).float()
        fy = torch.from_numpy(ys[..., 0]).float()
        flow = torch.stack([fx, fy], dim=1)          # (T, 2, H, W) in [0,255]
        flow = flow / 255.0 * 40.0 - 20.0
        x = T.resize_improved(flow, RESIZE_SIDE, smaller_edge=True)
        return x.to(device=device, dtype=dtype)

    def prepare(self, video_path):
        vid = video_path[0] if isinstance(video_path, tuple) else video_path
        return self._read_raw_frames(vid)

    # ------------------------------------------------------------ extract
    def extract(self, device: torch.device, models,
                video_path, prepared=None) -> Dict[str, np.ndarray]:
        precomputed = isinstance(video_path, tuple)
        vid_path = video_path[0] if precomputed else video_path
        with self._prof('decode'):
            frames_u8, fps = (prepared if prepared is not None
                              else self._read_raw_frames(vid_path))
        dtype = self.compute_dtype(device)
        n = frames_u8.shape[0]
        feats: Dict[str, List] = {s: [] for s in self.streams}
        ts: List[float] = []
        flow_all: Optional[torch.Tensor] = None
        if precomputed and 'flow' in self.streams:
            flow_all = self._read_precomputed_flow(video_path[1], device,
                                                   dtype, n - 1)
        ssz, step = self.stack_size, self.step_size
        starts = [s for s in range(0, max(n - ssz, 1), step)
                  if s + ssz + 1 <= n]
        # temporal parallelism: this rank owns every tp_world-th window
        # (merged back in rank order by runtime.dist.merge_temporal_shards)
        starts = starts[self.cfg.tp_rank::self.cfg.tp_world]
        bs = max(1, self.cfg.batch_size or 1)
        for i in range(0, len(starts), bs):
            grp = starts[i:i + bs]
            # (B, S+1, 3, H, W): batch of sliding windows — one flow-net
            # forward over all pairs, one I3D forward per stream; uploaded
            # as u8 and resized ON the device
            su8 = torch.stack([frames_u8[s:s + ssz + 1] for s in grp])
            su8 = su8.to(device=device, non_blocking=True)
            b, s1 = su8.shape[0], su8.shape[1]
            flat = su8.reshape(-1, *su8.shape[2:]).permute(0, 3, 1, 2).float()
            flat = T.resize_improved(flat, RESIZE_SIDE, smaller_edge=True)
            stacks = flat.reshape(b, s1, *flat.shape[1:]).to(dtype)
            for stream in self.streams:
                if stream == 'rgb':
                    x = T.center_crop(
                        stacks[:, :-1].reshape(-1, *stacks.shape[2:]), CROP)
                    x = T.scale_to_pm1(x)
                else:
                    if flow_all is not None:
                        flow = torch.cat([flow_all[s:s + ssz] for s in grp])
                    else:
                        with self._prof('flow'):
                            flow = self._compute_flow(models, stacks)
                    x = T.i3d_flow_preprocess(flow, CROP)
                clip = x.reshape(b, ssz, *x.shape[1:]).transpose(1, 2)
                with self._prof('infer'):
                    f = models[stream].forward_features(clip)
                feats[stream].append(f.float().cpu())
                if self.show_pred:
                    from ..utils.labels import show_predictions_on_dataset
                    logits = models[stream](clip).float().cpu()
                    for j, s0 in enumerate(grp):
                        print(f'{stream} stack @ {s0}:')
                        show_predictions_on_dataset(logits[j:j + 1],
                                                    'kinetics')
            ts.extend(s / fps * 1000.0 for s in grp)
        out: Dict[str, np.ndarray] = {
            s: (torch.cat(feats[s]).numpy() if feats[s]
                else np.zeros((0, I3D.FEAT_DIM), np.float32))
            for s in self.streams}
        out['fps'] = np.array(fps)
        out['timestamps_ms'] = np.array(ts)
        return out
