"""The reference's ``Inference`` engine (src/temporal/inference.py:19-191) with an MI355X slot: ``'gpu_mi355x'``.

``select_inference_engine`` (inference.py:46-80) asserts one of the reference's four device names and builds a
``SPETorch`` / Jetson engine; here the same class accepts ``'gpu_mi355x'`` and builds ``SPEMi355x`` (the drop-in
for ``SPETorch.predict``), so the GUI and the temporal tools (``TemporalPDF.update_pdf``, pdf_compare.py:94) run
on the new target. The reference's own devices can be served through ``engine_factories`` (device name ->
``factory(model, spe_utils)`` returning an object with ``predict``), e.g. the reference ``SPETorch`` for
'gpu_host' / 'cpu_host'; without a factory they raise, since those targets are the reference's, not this one's.

``predict`` keeps the reference's post-processing exactly: batch squeeze, quaternion pole continuity against the
previous still frame (:136-144), keypoints / bounding box for visualisation (:146-155), and the optional
'Adaptative' video filter (:158-190) -- whose filtered PDFs are decoded on the GPU (``Engine.decode`` on
``log(pdf)``: its softmax returns the PDF).

``predict_sequence`` is the same loop for T consecutive frames of one video in one call: one batched forward, one
decode and one video-filter step on the device (csrc/k_video.hip), sharing its state with ``predict``.

``video_type='Tracker'`` (both calls; not in the reference, which ships a Kalman filter it never wires in) tracks the
pose of any head, keypoint mode included, with the device tracker (csrc/k_track.hip, ``Engine.tracker``):
``pose_video`` = {'ori', 'pos', 'mahalanobis', 'track_status', 'keypoints', 'bbox'}. Its parameters are
``Inference.tracker_params``; its state lives on the device and ``reset()`` clears it. ``Inference.tracker_pdf_cov``
(off by default) makes the measurement covariance that of the soft-classification PDFs (``Engine.decode_cov``).
``Inference.tracker_modes = K`` (0 by default) keeps up to K orientations of an ambiguous orientation PDF per frame
(``Engine.decode_modes``) and lets the tracker pick among them; the still pose then carries 'modes'.

``video_type='Smoother'`` (``predict_sequence`` only: a recorded video) is the tracker followed by a fixed-interval
smoother over the T frames of the call (csrc/k_smooth.hip, ``PoseHistory.smooth``): ``pose_video`` is the smoothed pose
and also has 'smooth_status'. ``predict`` raises ValueError for it: a single frame has nothing to smooth.

``video_type='TrackerROI'`` (``predict_sequence`` only, keypoint mode only) is the tracker on raw camera frames, uint8
[T, Hin, Win, 3], with a track-guided region of interest (``SPEMi355x.predict_tracked_roi``): each frame is cropped to
the box of the pose the tracker predicts for it and resized to ``Inference.roi_size`` = (H, W), the network input, and
the keypoints are mapped back to the full frame before EPnP. ``Inference.roi_params``: margin, min_side. Both poses
also hold 'roi' (x0, y0, x1, y1) and 'roi_status'.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from .engine import Engine
from .spe_mi355x import SPEMi355x
from .temporal import TemporalPDF

REFERENCE_DEVICES = ('gpu_host', 'cpu_host', 'gpu_jetson', 'cpu_ultra96')   # inference.py:47
DEVICES = REFERENCE_DEVICES + ('gpu_mi355x',)


def model_to_blob(model, dtype: str = 'fp16'):
    """What ``SPEMi355x`` accepts: a packed blob (bytes / path / Engine) passes through; a torch ``nn.Module``
    (the reference's ``ModelWrapper``) or a reference-layout state_dict is BN-folded and packed (spef_amd.blob)."""
    if isinstance(model, (bytes, bytearray, str, Engine)):
        return model
    from . import blob
    sd = model.state_dict() if hasattr(model, 'state_dict') else model
    sd = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in sd.items()}
    return blob.pack(sd, dtype=dtype)


class Inference:
    def __init__(self, model, inference_device: str, spe_utils, device: str = 'cuda:0', dtype: str = 'fp16',
                 engine_factories: Optional[Dict[str, Callable]] = None):
        """Same arguments as the reference (inference.py:20-44); ``device`` / ``dtype`` select the MI355X GPU
        and the blob precision when ``model`` still has to be packed."""
        self.model = model
        self.inference_device = inference_device
        self.spe_utils = spe_utils
        self.inference_engine = None
        self.prev_still_ori = None
        self.prev_video_ori = None
        self.pdf_adapt_ori = TemporalPDF(n=0.8, alpha=16.49, distance_metric='l2')    # inference.py:38-39
        self.pdf_adapt_pos = TemporalPDF(n=0.5, alpha=48.64, distance_metric='l2')
        self.tracker_params = {}     # video_type 'Tracker': the parameters of Engine.tracker (q, p0, r, gate_chi2, ...)
        self.tracker_pdf_cov = False  # video_type 'Tracker': SPEMi355x.predict_tracked(pdf_cov=True), the PDFs' covariance
        self.tracker_modes = 0       # video_type 'Tracker': predict_tracked(modes=K), up to K orientation hypotheses per frame
        self.roi_size = None         # video_type 'TrackerROI': the network input (H, W) the crops are resized to
        self.roi_params = {}         # video_type 'TrackerROI': margin, min_side of SPEMi355x.predict_tracked_roi
        self.img_size = None
        self.device = device
        self.dtype = dtype
        self.engine_factories = dict(engine_factories or {})
        self.select_inference_engine(self.inference_device)

    def select_inference_engine(self, device: str, model_name: str = None) -> None:
        assert device in DEVICES
        self.close()
        self.inference_device = device
        if device == 'gpu_mi355x':
            self.inference_engine = SPEMi355x(model_to_blob(self.model, self.dtype), self.device, self.spe_utils)
        elif device in self.engine_factories:
            self.inference_engine = self.engine_factories[device](self.model, self.spe_utils)
        else:
            raise ValueError(f"inference device '{device}' is one of the reference's own targets: pass its engine "
                             f"through engine_factories, or use 'gpu_mi355x'")

    def close(self) -> None:
        if self.inference_engine is not None and hasattr(self.inference_engine, 'close'):
            self.inference_engine.close()
        self.inference_engine = None

    def reset(self) -> None:
        """inference.py:93-101."""
        self.prev_still_ori = None
        self.prev_video_ori = None
        self.pdf_adapt_ori.reset()
        self.pdf_adapt_pos.reset()
        eng = self.inference_engine
        if getattr(eng, '_track', None) is not None:     # video_type 'Tracker': the state lives on the device
            eng._track[1].reset()

    def update(self, model, spe_utils) -> None:
        """inference.py:103-115."""
        self.model = model
        self.spe_utils = spe_utils
        self.select_inference_engine(self.inference_device)
        self.reset()

    # ------------------------------------------------------------------ per frame
    def _visual(self, pose: dict) -> None:
        """Keypoints / bounding box for visualisation (inference.py:146-155)."""
        su = self.spe_utils
        if su.keypoints is None:
            return
        if su.ori_mode == 'keypoints' and su.pos_mode == 'keypoints':
            pose['bbox'] = su.keypoints.create_bbox_from_keypoints(pose['keypoints'])
        elif su.pos_mode in ('classification', 'regression') and su.ori_mode in ('classification', 'regression'):
            pose['keypoints'] = su.keypoints.create_keypoints2d(pose['ori'], pose['pos'])
            pose['bbox'] = su.keypoints.create_bbox_from_keypoints(pose['keypoints'])

    def _decode_pdfs(self, ori_pdf: np.ndarray, pos_pdf: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """orientation.decode / position.decode of one filtered PDF pair (inference.py:167-168), on the GPU: the
        decode kernels' softmax of log(pdf) is the PDF itself."""
        eng = self.inference_engine.engine
        dev = eng.device
        with np.errstate(divide='ignore'):
            lo = torch.from_numpy(np.log(ori_pdf.astype(np.float32))[None].copy()).to(dev)
            lp = torch.from_numpy(np.log(pos_pdf.astype(np.float32))[None].copy()).to(dev)
        dec = eng.decode(L.CLASSIFICATION, L.CLASSIFICATION, lo, lp)
        st = dec['status'].cpu().numpy()
        if st.any():
            raise ValueError('Weighted PDF contains NaN or sums to zero')   # classification_utils.py:134-135, 253
        return dec['ori'][0].cpu().numpy(), dec['pos'][0].cpu().numpy()

    def _still_pole(self, ori: np.ndarray) -> np.ndarray:
        """The pole rule of ``predict`` over a run of still quaternions [T x 4], on the host -> the run, flipped."""
        ori = np.array(ori, copy=True)
        for t in range(ori.shape[0]):
            if self.prev_still_ori is None:
                self.prev_still_ori = ori[t]
                continue
            dot = np.dot(self.prev_still_ori, ori[t])
            if dot < 0:
                ori[t] = -ori[t]
            if np.abs(dot) > 0.5:
                self.prev_still_ori = ori[t]
        return ori

    def _tracked(self, images: torch.Tensor, smooth: bool = False, roi: bool = False) -> list:
        """video_type 'Tracker' for T consecutive frames of one video: one batched forward, one decode and one
        tracker step on the GPU (``SPEMi355x.predict_tracked``, one stream; the state stays in the device tracker, so
        any cut of a video into calls gives the same poses). -> T triples (pose_still, latency_ms, pose_video) with
        pose_video = {'ori', 'pos', 'mahalanobis', 'track_status', 'keypoints', 'bbox'}; in keypoint mode its
        'keypoints' are the reprojection of the tracked pose. With ``smooth`` (video_type 'Smoother') the pose is the
        fixed-interval smoother's over these T frames and pose_video also has 'smooth_status'. With ``roi`` (video_type
        'TrackerROI') ``images`` are raw uint8 frames [T, Hin, Win, 3] and the loop is ``predict_tracked_roi``'s."""
        eng, su = self.inference_engine, self.spe_utils
        if not hasattr(eng, 'predict_tracked'):
            raise ValueError("video filtering 'Tracker' needs the 'gpu_mi355x' engine")
        T = int(images.shape[0])
        pdf_cov = {'pdf_cov': True} if self.tracker_pdf_cov else {}
        modes = {'modes': int(self.tracker_modes)} if self.tracker_modes else {}
        smoothing = {'smooth': True} if smooth else {}
        if roi:
            if self.roi_size is None:
                raise ValueError("video filtering 'TrackerROI' needs Inference.roi_size = (H, W), the network input")
            still, tracked, latency_ms = eng.predict_tracked_roi(images, self.roi_size, 1, **self.roi_params,
                                                                 **self.tracker_params)
        else:
            still, tracked, latency_ms = eng.predict_tracked(images, 1, **pdf_cov, **modes, **smoothing,
                                                             **self.tracker_params)
        still = dict(still)
        still['ori'] = self._still_pole(still['ori'])
        found = still.pop('modes', None)     # tracker_modes: a dict of per-frame arrays
        out = []
        for t in range(T):
            pose_still = {k: v[t] for k, v in still.items()}
            if found is not None:
                pose_still['modes'] = {k: v[t] for k, v in found.items()}
            self._visual(pose_still)
            pose_video = {k: v[t] for k, v in tracked.items()}
            if su.keypoints is not None:
                pose_video['keypoints'] = su.keypoints.create_keypoints2d(pose_video['ori'], pose_video['pos'])
                pose_video['bbox'] = su.keypoints.create_bbox_from_keypoints(pose_video['keypoints'])
            out.append((pose_still, latency_ms / T, pose_video))
        return out

    @staticmethod
    def _advance_pole(pole, quats: np.ndarray):
        """The pole after a run of quaternions that already follow it (the rule of ``predict``; no flips left)."""
        for q in quats:
            if pole is None or np.abs(np.dot(pole, q)) > 0.5:
                pole = q
        return pole

    def predict_sequence(self, images: torch.Tensor, video_type: Optional[str] = 'Adaptative') -> list:
        """``images`` [T, 3, H, W]: T consecutive frames of one video -> the list of T ``(pose_still, latency_ms,
        pose_video)`` triples that T calls of ``predict(images[t:t+1], video_type)`` return (keypoints and bounding
        box included), computed with one batched forward, one decode and one video-filter step on the GPU
        (``SPEMi355x.predict_video``; each frame is given latency / T). The reference runs this loop at batch 1
        (temporal.py:102). The state is the one ``predict`` uses: it is loaded into the device filter before the
        step and read back after it, so ``reset()`` clears both and the two calls can be mixed on one video.
        An engine without ``predict_video`` (one of the reference's own, through ``engine_factories``) is driven
        frame by frame."""
        if video_type == 'TrackerROI':              # raw frames; the tracker decides what the network sees
            if self.roi_size is not None:
                self.img_size = (1, 3) + tuple(int(v) for v in self.roi_size)
            return self._tracked(images, roi=True)
        if video_type in ('Tracker', 'Smoother'):   # 'Smoother': the tracker and a backward pass over these T frames
            self.img_size = (1,) + tuple(images.size())[1:]
            return self._tracked(images, smooth=video_type == 'Smoother')
        if video_type is not None and video_type != 'Adaptative':
            raise ValueError(f'type of video filtering not implemented: {video_type}')
        eng = self.inference_engine
        T = int(images.shape[0])
        if not hasattr(eng, 'predict_video'):
            return [self.predict(images[t:t + 1], video_type) for t in range(T)]
        self.img_size = (1,) + tuple(images.size())[1:]
        fo, fp = self.pdf_adapt_ori, self.pdf_adapt_pos
        video = None
        if video_type is None:
            still, latency_ms = eng.predict(images)
            still = dict(still)
            ori = np.array(still['ori'], copy=True)
            for t in range(T):                       # the pole rule of predict, on the host
                if self.prev_still_ori is None:
                    self.prev_still_ori = ori[t]
                    continue
                dot = np.dot(self.prev_still_ori, ori[t])
                if dot < 0:
                    ori[t] = -ori[t]
                if np.abs(dot) > 0.5:
                    self.prev_still_ori = ori[t]
            still['ori'] = ori
        else:
            assert self.spe_utils.ori_mode == 'classification'
            assert self.spe_utils.pos_mode == 'classification'
            if fo.distance_metric != fp.distance_metric:
                raise ValueError('the device filter uses one distance metric for both heads')
            params = dict(n_ori=fo.n, alpha_ori=fo.alpha, n_pos=fp.n, alpha_pos=fp.alpha)
            vf = eng.video_filter(1, fo.distance_metric, **params)
            vf.set_state(0, fo.previous_pdf, fp.previous_pdf, self.prev_still_ori, self.prev_video_ori)
            still, video, latency_ms = eng.predict_video(images, 1, fo.distance_metric, **params)
            fo.previous_pdf = np.array(video['ori_soft'][-1], copy=True)
            fp.previous_pdf = np.array(video['pos_soft'][-1], copy=True)
            self.prev_still_ori = self._advance_pole(self.prev_still_ori, still['ori'])
            self.prev_video_ori = self._advance_pole(self.prev_video_ori, video['ori'])
        out = []
        for t in range(T):
            pose_still = {k: v[t] for k, v in still.items()}
            self._visual(pose_still)
            pose_video = None
            if video is not None:
                pose_video = {k: v[t] for k, v in video.items()}
                self._visual(pose_video)
            out.append((pose_still, latency_ms / T, pose_video))
        return out

    def predict(self, image: torch.Tensor, video_type: str = None) -> Tuple[dict, float, Optional[dict]]:
        """inference.py:117-191: -> (pose of the still frame, latency ms, filtered video pose or None)."""
        if not self.img_size or self.img_size != tuple(image.size()):
            self.img_size = tuple(image.size())
        if video_type == 'Smoother':
            raise ValueError("video filtering 'Smoother' needs a recorded sequence (predict_sequence): a single frame "
                             'has nothing to smooth')
        if video_type == 'Tracker':      # the pose tracker (any head): still and tracked pose from one device pass
            return self._tracked(image)[0]
        pose_still, latency_ms = self.inference_engine.predict(image)
        pose_still = {k: v.squeeze(0) for k, v in pose_still.items()}
        if self.prev_still_ori is not None:   # no quaternion sign flips between frames
            dot = np.dot(self.prev_still_ori, pose_still['ori'])
            if dot < 0:
                pose_still['ori'] = -pose_still['ori']
            if np.abs(dot) > 0.5:            # an outlier does not move the pole
                self.prev_still_ori = pose_still['ori']
        else:
            self.prev_still_ori = pose_still['ori']
        self._visual(pose_still)

        pose_video = None
        if video_type is not None:
            if video_type != 'Adaptative':
                raise ValueError(f'type of video filtering not implemented: {video_type}')
            assert self.spe_utils.ori_mode == 'classification'
            assert self.spe_utils.pos_mode == 'classification'
            pose_video = {}
            pose_video['ori_soft'], pose_video['ori_distance'] = self.pdf_adapt_ori.update_pdf(pose_still['ori_soft'])
            pose_video['pos_soft'], pose_video['pos_distance'] = self.pdf_adapt_pos.update_pdf(pose_still['pos_soft'])
            pose_video['ori'], pose_video['pos'] = self._decode_pdfs(pose_video['ori_soft'], pose_video['pos_soft'])
            if self.prev_video_ori is not None:
                dot = np.dot(self.prev_video_ori, pose_video['ori'])
                if dot < 0:
                    pose_video['ori'] = -pose_video['ori']
                if np.abs(dot) > 0.5:
                    self.prev_video_ori = pose_video['ori']
            else:
                self.prev_video_ori = pose_video['ori']
            self._visual(pose_video)
        return pose_still, latency_ms, pose_video
