"""``SPEMi355x`` -- the MI355X inference target behind the reference's "SPE model" interface.

Drop-in for ``SPETorch`` (src/spe/spe_torch.py:12-124), ``SPETVMARM`` (src/tvm/spe_tvm.py:12) and
``SPEJetson`` (src/nvidia/spe_nvidia.py:53): same ``predict(images) -> (pose, latency_ms)`` contract, same
pose-dict keys, same exception types, so ``tools/evaluation.py:71`` and the ``deploy_*`` throughput loops
(``num_predict``, deploy_nvidia.py:93) call it unchanged.

Differences from SPETorch, all deliberate:
  * forward AND decode run on the GPU (HIP kernels); the reference decodes on the host in NumPy
    (spe_torch.py:73-74, classification_utils.py:163-164);
  * latency is measured with HIP events after a device sync (the reference's ``time.time()`` around an
    un-synchronised forward times only the launch, spe_torch.py:57-61);
  * ``num_predict`` > 1 repeats the device work and reports the mean, like SPEJetson's server loop
    (jetson_inference_server.py:129-141).
"""
from __future__ import annotations

import gc
from typing import Dict, Tuple, Union

import numpy as np
import torch

from . import _lib as L
from .engine import Engine

_MODES = {'regression': L.REGRESSION, 'classification': L.CLASSIFICATION, 'keypoints': L.KEYPOINTS}


class SPEMi355x:
    """Args:
        model: a weight blob (bytes, from build_mi355x.py / ``spef_amd.blob.pack``), a path to one, or an
            already-loaded ``Engine``.
        device: HIP device (``cuda:N``).
        spe_utils: the reference ``SPEUtils`` (or ``spef_amd.spe.spe_utils.SPEUtils``): provides ori/pos mode
            and the decode histograms.
        keypoint_refine: None (off) or ``(max_iters, huber_px)``: keypoint mode refines EPnP's pose by robust
            Levenberg-Marquardt on the GPU (``Engine.set_keypoint_refine``); ``predict`` then returns the refined
            'ori' / 'pos' and adds 'ori_epnp', 'pos_epnp' and 'reproj_rms' (px, before / after).
        keypoint_consensus: None (off) or ``(inlier_px, min_inliers)`` (``min_inliers`` 0 or None: the default,
            max(4, ceil(n / 2))): keypoint mode selects inliers by exhaustive 3-point consensus between EPnP and the
            refinement (``Engine.set_keypoint_consensus``); ``predict`` then also returns 'inliers', 'n_inliers',
            'ori_consensus' and 'pos_consensus'.
    """

    def __init__(self, model: Union[bytes, str, Engine], device: Union[str, torch.device], spe_utils,
                 keypoint_refine=None, keypoint_consensus=None) -> None:
        self.spe_utils = spe_utils
        self.keypoint_refine = tuple(keypoint_refine) if keypoint_refine and keypoint_refine[0] else None
        self.keypoint_consensus = None
        if keypoint_consensus and keypoint_consensus[0]:
            self.keypoint_consensus = (float(keypoint_consensus[0]),
                                       int(keypoint_consensus[1]) if len(keypoint_consensus) > 1 and
                                       keypoint_consensus[1] else None)
        self.device = torch.device(device)
        self.engine = None
        self._video = None          # (configuration, VideoFilter) of predict_video
        self._track = None          # (configuration, PoseTracker) of predict_tracked
        self._pipe = None           # StreamPipeline of evaluation_device
        self.update_model(model, self.device)

    # ------------------------------------------------------------------ lifecycle (spe_torch.py:78-124)
    def update_model(self, model, device) -> None:
        if self.engine is not None:
            self.delete_model()
        self.device = torch.device(device)
        if isinstance(model, Engine):
            self.engine = model
        else:
            if isinstance(model, str):
                with open(model, 'rb') as f:
                    model = f.read()
            self.engine = Engine(model, self.device)
        su = self.spe_utils
        self.ori_mode, self.pos_mode = _MODES[su.ori_mode], _MODES[su.pos_mode]
        self.keypoint_mode = self.ori_mode == L.KEYPOINTS and self.pos_mode == L.KEYPOINTS
        if (self.ori_mode == L.KEYPOINTS) != (self.pos_mode == L.KEYPOINTS):
            raise ValueError('keypoints mode must be used for both orientation and position')  # spe_utils.py:66
        if self.keypoint_mode:
            kp = su.keypoints
            if kp is None:
                raise ValueError('keypoints mode needs SPEUtils.keypoints (a KeyPoints with keypoints3d)')
            cam = kp.camera
            self.engine.set_keypoints(np.asarray(kp.keypoints3d, np.float32), np.asarray(cam.K, np.float64),
                                      float(cam.nu), float(cam.nv), getattr(cam, 'distCoeffs', None))
            if self.engine.n_out0 != 2 * (kp.keypoints3d.shape[0] + 1):   # model.py:236
                raise AssertionError(f'keypoint head width {self.engine.n_out0} != 2 * (n_keypoints + 1)')
            if self.keypoint_refine is not None:
                self.engine.set_keypoint_refine(*self.keypoint_refine)
            if self.keypoint_consensus is not None:
                self.engine.set_keypoint_consensus(*self.keypoint_consensus)
            return
        ori_bins = su.orientation.histogram if self.ori_mode == L.CLASSIFICATION else None
        pos_grid = su.position.histogram if self.pos_mode == L.CLASSIFICATION else None
        self.engine.set_decode_tables(ori_bins, pos_grid)
        # the head widths in the blob must agree with the decode configuration (model.py:225-234)
        want0 = su.orientation.n_bins if self.ori_mode == L.CLASSIFICATION else 4
        want1 = su.position.n_bins if self.pos_mode == L.CLASSIFICATION else 3
        # (raised, not asserted: python -O must not drop it; spef_decode re-checks the widths in C as well)
        if (self.engine.n_out0, self.engine.n_out1) != (want0, want1):
            raise AssertionError(f'model head {(self.engine.n_out0, self.engine.n_out1)} != decode config '
                                 f'{(want0, want1)}')

    def delete_model(self) -> None:
        self._close_video()
        self._close_track()
        self._close_pipe()
        if self.engine is not None:
            self.engine.close()
        self.engine = None
        gc.collect()

    def close(self) -> None:
        self.delete_model()

    # ------------------------------------------------------------------ inference
    def _run(self, x: torch.Tensor, want_cov: bool = False):
        raw0, raw1 = self.engine.forward(x)
        if self.keypoint_mode:   # sigmoid + batched EPnP on the GPU (spe_utils.py:66-68, keypoints_utils.py:152)
            return raw0, None, self.engine.decode_keypoints(raw0, apply_sigmoid=True, want_cov=want_cov)
        if want_cov:
            return raw0, raw1, self.engine.decode(self.ori_mode, self.pos_mode, raw0, raw1, want_cov=True,
                                                  want_hinv=self.ori_mode == L.CLASSIFICATION)
        return raw0, raw1, self.engine.decode(self.ori_mode, self.pos_mode, raw0, raw1)

    def predict_frames(self, frames: torch.Tensor, img_size, num_predict: int = 1) -> Tuple[Dict, float]:
        """Raw decoded camera frames (uint8 [B, Hin, Win, 3], e.g. 1200 x 1920 SPEED images converted to RGB)
        -> the pose dict: the DataLoader's ``Resize(img_size)`` + ``ToTensor`` (speed.py:66-69, utils.py:212-249)
        run on the GPU (bit-identical to Pillow's BILINEAR resize), then ``predict``. Latency covers both."""
        x = frames.to(self.device, non_blocking=True).contiguous()
        torch.cuda.synchronize(self.device)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(max(1, num_predict)):
            small = self.engine.preprocess(x, img_size)
            raw0, raw1, dec = self._run(small)
        end.record()
        end.synchronize()
        return self._pose(dec), start.elapsed_time(end) / max(1, num_predict)

    def predict(self, images: torch.Tensor, num_predict: int = 1, want_cov: bool = False) -> Tuple[Dict, float]:
        """images: NCHW float32 in [0,1] (the reference ``images['torch']``) or NHWC uint8 frames.
        ``want_cov`` (off by default): the pose dict also has 'cov' [B x 6 x 6], the pose covariance of the
        soft-classification PDFs (``Engine.decode_cov``; order theta, t; a regression head's block is the default
        fixed variance), its 'cov_status' and, behind an orientation classification head, 'ori_hinv' [B x 4 x 4], the
        second value of the reference's orientation decode. In keypoint mode with ``keypoint_refine`` 'cov' is the
        refinement's."""
        if self.engine is None:
            raise AssertionError('no model loaded')            # spe_torch.py:55 (assert hasattr(self, 'model'))
        x = images.to(self.device, non_blocking=True).contiguous()
        torch.cuda.synchronize(self.device)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(max(1, num_predict)):
            raw0, raw1, dec = self._run(x, want_cov)
        end.record()
        end.synchronize()
        latency_ms = start.elapsed_time(end) / max(1, num_predict)
        return self._pose(dec, want_cov=want_cov), latency_ms

    # ------------------------------------------------------------------ video
    def video_filter(self, n_streams: int = 1, metric: str = 'l2', **params):
        """The engine's ``VideoFilter`` for this configuration (created on first use, kept with its state until
        the configuration changes or the model is deleted). ``params``: n_ori, alpha_ori, n_pos, alpha_pos."""
        key = (int(n_streams), metric.lower(), tuple(sorted(params.items())))
        if self._video is None or self._video[0] != key:
            self._close_video()
            self._video = (key, self.engine.video_filter(n_streams, metric, **params))
        return self._video[1]

    def _close_video(self) -> None:
        if getattr(self, '_video', None) is not None:
            self._video[1].close()
        self._video = None

    def eval_pipeline(self, depth: int = 3):
        """A ``StreamPipeline`` of ``depth`` further contexts holding this model's weights and decode configuration
        (``evaluation_device`` drives it); created on first use, closed with the model."""
        from .pipeline import StreamPipeline
        if self._pipe is None or self._pipe.depth != depth:
            self._close_pipe()
            if self.engine.blob is None:
                raise AssertionError('the engine does not hold its weight blob (weights received by broadcast)')
            tables = self.engine._decode_tables or (None, None)
            self._pipe = StreamPipeline(self.engine.blob, self.device, depth, *tables)
            if self.keypoint_mode:
                kp, kk, dd = self.engine._kp
                cam = self.spe_utils.keypoints.camera
                self._pipe.set_keypoints(kp, kk.reshape(3, 3), float(cam.nu), float(cam.nv), dd if dd.size else None)
                if self.keypoint_refine is not None:
                    self._pipe.set_keypoint_refine(*self.keypoint_refine)
                if self.keypoint_consensus is not None:
                    self._pipe.set_keypoint_consensus(*self.keypoint_consensus)
        return self._pipe

    def _close_pipe(self) -> None:
        if getattr(self, '_pipe', None) is not None:
            self._pipe.close()
        self._pipe = None

    def predict_video(self, images: torch.Tensor, n_streams: int = 1, metric: str = 'l2', targets=None, scorer=None,
                      **params) -> Tuple[Dict, Dict, float]:
        """Time-major video frames ``images`` [T * n_streams, 3, H, W] (row t * n_streams + s = step t of stream
        s) -> (still pose, video pose, latency ms): one batched forward, one decode and one video-filter step, all
        on the GPU. Both are batched NumPy dicts with the keys of ``Inference.predict``: the still pose has 'ori',
        'pos', 'ori_soft', 'pos_soft'; the video pose adds 'ori_distance' / 'pos_distance' and holds the filtered
        PDFs and their decode. The quaternions of both follow their stream's pole (inference.py:136-144). The
        filter's state persists between calls (``video_filter(...).reset()`` starts new videos).
        With ``targets`` ({'ori', 'pos'} of the frames) and ``scorer`` (``engine.scorer(n_streams, 2, capacity)``)
        both poses are scored on the device as well: track 0 logs the still poses and track 1 the filtered ones, one
        group per stream; ``scorer.result()`` then gives the still against filtered statistics per video."""
        if self.engine is None:
            raise AssertionError('no model loaded')
        if self.ori_mode != L.CLASSIFICATION or self.pos_mode != L.CLASSIFICATION:
            raise AssertionError('the video filter needs classification heads (soft PDFs)')   # inference.py:161-162
        x = images.to(self.device, non_blocking=True).contiguous()
        B = x.shape[0]
        if n_streams < 1 or B % n_streams:
            raise AssertionError(f'{B} frames are not whole time steps of {n_streams} streams')
        vf = self.video_filter(n_streams, metric, **params)
        torch.cuda.synchronize(self.device)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        _, _, dec = self._run(x)
        vid = vf.step(dec, B // n_streams)
        if targets is not None and scorer is not None:
            if scorer.n_groups != n_streams or scorer.n_tracks < 2:
                raise AssertionError(f'the scorer needs {n_streams} groups and 2 tracks')
            tg = scorer.targets(targets)
            scorer.step(0, dec, tg, B // n_streams)
            scorer.step(1, vid, tg, B // n_streams)
        end.record()
        end.synchronize()
        still = self._pose(dec)
        if np.any(vid['status'].cpu().numpy()):
            raise ValueError('Weighted PDF contains NaN or sums to zero')   # classification_utils.py:134-135, 253
        video = {k: vid[k].cpu().numpy() for k in ('ori', 'pos', 'ori_soft', 'pos_soft', 'ori_distance',
                                                   'pos_distance')}
        return still, video, start.elapsed_time(end)

    # ------------------------------------------------------------------ tracking
    def tracker(self, n_streams: int = 1, **params):
        """The engine's ``PoseTracker`` for this configuration (created on first use, kept with its state until the
        configuration changes or the model is deleted). ``params``: q, p0, r, cov_scale, gate_chi2, max_coast."""
        key = (int(n_streams), tuple(sorted((k, tuple(np.atleast_1d(v).tolist())) for k, v in params.items())))
        if self._track is None or self._track[0] != key:
            self._close_track()
            self._track = (key, self.engine.tracker(n_streams, **params))
        return self._track[1]

    def _history(self, trk, capacity: int):
        """The ``PoseHistory`` of ``predict_tracked(smooth=True)``: kept with the tracker, grown when a call is longer."""
        h = getattr(self, '_hist', None)
        if h is None or h.tracker is not trk or h.capacity < capacity:
            if h is not None:
                h.close()
            self._hist = h = trk.history(capacity)
        return h

    def _close_track(self) -> None:
        if getattr(self, '_hist', None) is not None:
            self._hist.close()
        self._hist = None
        if getattr(self, '_track', None) is not None:
            self._track[1].close()
        self._track = None

    def predict_tracked(self, images: torch.Tensor, n_streams: int = 1, targets=None, scorer=None,
                        pdf_cov: bool = False, floor_var=(0.0, 0.0), modes: int = 0, modes_params=None,
                        smooth: bool = False, **params) -> Tuple[Dict, Dict, float]:
        """Time-major video frames ``images`` [T * n_streams, ...] (row t * n_streams + s = step t of stream s) ->
        (still pose, tracked pose, latency ms) for every head mode: one batched forward, one decode and one tracker
        step (``Engine.tracker``: an error-state Kalman filter with gating and coasting), all on the GPU. The still
        pose is what ``predict`` returns, except that a row whose decode failed does not raise here: the tracker coasts
        over it and reports it in ``tracked['track_status']`` (bit 1; with bit 8 when the stream has no track yet and the
        row passes through). The tracked pose has 'ori', 'pos', 'mahalanobis' and 'track_status'. In keypoint mode with
        ``keypoint_refine`` or ``keypoint_consensus`` the refined pose's covariance (which counts the inliers only) is the
        measurement covariance. Behind the URSONet heads
        ``pdf_cov=True`` makes it the covariance of the soft-classification PDFs about their own decode
        (``Engine.decode_cov`` with ``fixed_var`` = the tracker's ``r`` for a regression head and ``floor_var`` added to
        a classification head's diagonal; a row whose PDF gives no covariance falls back to ``r``), which lets a
        Mahalanobis gate fire; otherwise (the default) the fixed ``r`` is.
        ``modes=K`` (1..4; 0, the default, is the path above, untouched) keeps up to K orientations of an ambiguous
        orientation PDF and lets the tracker pick: decode -> ``decode_cov`` -> ``Engine.decode_modes`` (``modes_params``:
        sep_deg, seed_rel, min_mass, rounds) -> ``PoseTracker.step_modes``. The still pose then has 'modes' = {'quat'
        [B x K x 4], 'mass' [B x K], 'n' [B], 'chosen' [B]} and the tracked pose 'chosen'. It needs a classification
        orientation head (AssertionError otherwise).
        The tracker's state persists between calls (``tracker(...).reset()`` starts new videos). ``params``: as
        ``Engine.tracker``. With ``targets`` and ``scorer`` (``engine.scorer(n_streams, 2, capacity)``) track 0 logs the
        still poses and track 1 the tracked ones; a tracked row counts as failed only where it passed through.
        ``smooth=True`` (a recorded video): the posteriors of the call's T frames are recorded on the device and a
        fixed-interval smoother (``PoseHistory.smooth``: a Rauch-Tung-Striebel backward pass; the window is this call)
        replaces 'ori' and 'pos' of the tracked pose by the smoothed ones, adds 'smooth_status' and is what a scorer
        scores as track 1; 'mahalanobis' and 'track_status' stay the filter's, and so does the tracker's state. With
        ``modes=K`` the frames are recorded through ``PoseHistory.push``, one ``step_modes`` per time step (the same
        track bit for bit: a stream's result does not depend on how its frames are cut into calls)."""
        if self.engine is None:
            raise AssertionError('no model loaded')
        x = images.to(self.device, non_blocking=True).contiguous()
        B = x.shape[0]
        if n_streams < 1 or B % n_streams:
            raise AssertionError(f'{B} frames are not whole time steps of {n_streams} streams')
        modes = int(modes)
        if modes and (self.keypoint_mode or self.ori_mode != L.CLASSIFICATION):
            raise AssertionError('modes needs a classification orientation head (a soft PDF)')
        if modes < 0 or modes > L.MODES_MAX:
            raise AssertionError(f'modes must be in 0..{L.MODES_MAX}')
        trk = self.tracker(n_streams, **params)
        torch.cuda.synchronize(self.device)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        raw0, raw1 = self.engine.forward(x)
        if modes:
            dec = self.engine.decode(self.ori_mode, self.pos_mode, raw0, raw1, want_cov=True, fixed_var=trk.params['r'],
                                     floor_var=floor_var)
            self.engine.decode_modes(dec, k_max=modes, floor_var=float(np.asarray(floor_var).reshape(-1)[0]),
                                     **(modes_params or {}))
        elif self.keypoint_mode:
            dec = self.engine.decode_keypoints(raw0, apply_sigmoid=True, want_cov=self.keypoint_refine is not None or
                                               self.keypoint_consensus is not None)
        elif pdf_cov:
            dec = self.engine.decode(self.ori_mode, self.pos_mode, raw0, raw1, want_cov=True, fixed_var=trk.params['r'],
                                     floor_var=floor_var)
        else:
            dec = self.engine.decode(self.ori_mode, self.pos_mode, raw0, raw1)
        T = B // n_streams
        if not smooth:
            out = trk.step_modes(dec, T) if modes else trk.step(dec, T)
        else:
            hist = self._history(trk, T)
            hist.reset()
            if modes:
                keys = [k for k, v in dec.items() if isinstance(v, torch.Tensor) and v.shape[:1] == (B,)]
                parts = []
                for t in range(T):
                    rows = slice(t * n_streams, (t + 1) * n_streams)
                    parts.append(trk.step_modes({k: dec[k][rows] for k in keys}, 1))
                    hist.push(parts[-1]['track_status'])
                out = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
            else:
                out = trk.step(dec, T, history=hist)
            sm = hist.smooth(out)
            out = dict(out, ori=sm['ori'], pos=sm['pos'], smooth_status=sm['smooth_status'])
        if targets is not None and scorer is not None:
            if scorer.n_groups != n_streams or scorer.n_tracks < 2:
                raise AssertionError(f'the scorer needs {n_streams} groups and 2 tracks')
            tg = scorer.targets(targets)
            scorer.step(0, dict(dec, status=dec['status'] & 15), tg, B // n_streams)
            scorer.step(1, dict(out, status=out['track_status'] & 8), tg, B // n_streams)
        end.record()
        end.synchronize()
        tracked = {k: out[k].cpu().numpy() for k in ('ori', 'pos', 'mahalanobis', 'track_status') +
                   (('smooth_status',) if smooth else ())}
        still = self._pose(dec, check=False)
        if modes:
            tracked['chosen'] = out['chosen'].cpu().numpy()
            still['modes'] = {'quat': dec['mode_quat'].cpu().numpy(), 'mass': dec['mode_mass'].cpu().numpy(),
                              'n': dec['n_modes'].cpu().numpy(), 'chosen': tracked['chosen']}
        return still, tracked, start.elapsed_time(end)

    def predict_tracked_roi(self, frames: torch.Tensor, img_size, n_streams: int = 1, margin: float = 0.2,
                            min_side: float = 32.0, **params) -> Tuple[Dict, Dict, float]:
        """``predict_tracked`` on raw camera frames with a track-guided region of interest, keypoint mode only
        (ValueError otherwise): ``frames`` uint8 [T * n_streams, Hin, Win, 3], time-major. The network sees, per frame,
        the box of the pose the tracker predicts for it (``Engine.roi_boxes``: the projected model grown by ``margin``,
        at least ``min_side`` px, at the aspect of ``img_size``) cropped and resized to ``img_size`` = (H, W); the
        keypoints it gives are mapped back to the full frame before EPnP, so the head's error costs box width / nu as
        many pixels. The first frame of a stream, and every frame while it has no track, gets the full frame through
        the same kernels. Time is sequential by nature: per step predict -> boxes -> crop-resize of the step's
        ``n_streams`` frames -> forward -> un-map -> ``decode_keypoints(apply_sigmoid=False)`` with the configured
        consensus and refinement -> ``tracker.step(T=1)``, all enqueued on one stream with no host synchronisation
        inside the loop. -> (still pose, tracked pose, latency ms) as ``predict_tracked``; both dicts also hold 'roi'
        [T * n_streams x 4] int32 (x0, y0, x1, y1) and 'roi_status' (bit 1: full frame). The model must have been
        trained on such crops; training is not this project's. ``params``: as
        ``Engine.tracker``."""
        if self.engine is None:
            raise AssertionError('no model loaded')
        if not self.keypoint_mode:
            raise ValueError('predict_tracked_roi needs keypoint mode: a crop under a soft-classification head '
                             'changes the apparent attitude')
        x = frames.to(self.device, non_blocking=True).contiguous()
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise AssertionError('frames must be raw uint8 [T * n_streams, Hin, Win, 3]')
        B, S = x.shape[0], int(n_streams)
        if S < 1 or B % S:
            raise AssertionError(f'{B} frames are not whole time steps of {S} streams')
        T, eng = B // S, self.engine
        frame_size, size = (x.shape[1], x.shape[2]), (int(img_size[0]), int(img_size[1]))
        want_cov = self.keypoint_refine is not None or self.keypoint_consensus is not None
        trk = self.tracker(S, **params)
        torch.cuda.synchronize(self.device)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        decs, outs, rois, stats = [], [], [], []
        for t in range(T):
            pred = trk.predict()
            box, bst = eng.roi_boxes(pred['ori'], pred['pos'], frame_size, size, margin, min_side, have=pred['have'])
            small = eng.preprocess_roi(x[t * S:(t + 1) * S], box, size)
            raw0, _ = eng.forward(small)
            kp = eng.unmap_keypoints(raw0, box, apply_sigmoid=True)
            dec = eng.decode_keypoints(kp, apply_sigmoid=False, want_cov=want_cov)
            outs.append(trk.step(dec, 1))
            decs.append(dec)
            rois.append(box)
            stats.append(bst)
        end.record()
        end.synchronize()
        dec = {k: torch.cat([d[k] for d in decs]) for k in decs[0]}
        out = {k: torch.cat([o[k] for o in outs]) for k in outs[0]}
        roi, roi_status = torch.cat(rois).cpu().numpy(), torch.cat(stats).cpu().numpy()
        tracked = {k: out[k].cpu().numpy() for k in ('ori', 'pos', 'mahalanobis', 'track_status')}
        still = self._pose(dec, check=False)
        for d in (still, tracked):
            d['roi'], d['roi_status'] = roi, roi_status
        return still, tracked, start.elapsed_time(end)

    def _pose(self, dec, check: bool = True, want_cov: bool = False) -> Dict:
        status = dec['status'].cpu().numpy() if check else np.zeros(1, np.int32)
        if np.any(status & 1):
            raise ValueError('Error during orientation decoding')                       # classification_utils.py:135
        if np.any(status & 2):
            raise ValueError('Encoded position vector sum is zero, cannot decode.')     # :254
        if np.any(status & 4):
            raise ValueError('Error during position decoding, NaN found in decoded position.')  # :263
        if np.any(status & 8):
            raise ValueError('EPnP failed on a batch row (degenerate keypoints)')   # cv2.solvePnP error analogue

        # bits 16 (row not refined), 32 (refinement stopped at max_iters) and 64 (no consensus) are informational: the
        # pose stands
        if self.keypoint_mode:
            pose = {'keypoints': dec['keypoints'].cpu().numpy(), 'ori': dec['ori'].cpu().numpy(),
                    'pos': dec['pos'].cpu().numpy()}
            if 'ori_epnp' in dec:   # keypoint_refine
                pose['ori_epnp'] = dec['ori_epnp'].cpu().numpy()
                pose['pos_epnp'] = dec['pos_epnp'].cpu().numpy()
                pose['reproj_rms'] = dec['fit'][:, :2].cpu().numpy()
            for k in ('inliers', 'n_inliers', 'ori_consensus', 'pos_consensus'):   # keypoint_consensus
                if k in dec:
                    pose[k] = dec[k].cpu().numpy()
            if want_cov and 'cov' in dec:
                pose['cov'] = dec['cov'].cpu().numpy()
            return pose

        pose = {'ori': dec['ori'].cpu().numpy(), 'pos': dec['pos'].cpu().numpy()}
        if self.ori_mode == L.CLASSIFICATION:
            pose['ori_soft'] = dec['ori_soft'].cpu().numpy()
        if self.pos_mode == L.CLASSIFICATION:
            pose['pos_soft'] = dec['pos_soft'].cpu().numpy()
        for k in ('cov', 'cov_status', 'ori_hinv') if want_cov else ():
            if k in dec:
                pose[k] = dec[k].cpu().numpy()
        return pose
