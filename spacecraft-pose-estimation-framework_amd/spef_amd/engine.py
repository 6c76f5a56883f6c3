"""Device-side engine: one SPEF context (one GPU) driven through the C ABI.

PyTorch-ROCm is plumbing here: it owns device memory (output tensors) and the current HIP stream;
every computation is a HIP kernel in libspef_mi355x.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib as L


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device: torch.device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class VideoFilter:
    """Device state of the adaptive video filter for ``n_streams`` streams (``Engine.video_filter``).

    Frames are time-major: a batch of ``T * n_streams`` rows holds T consecutive time steps of every stream, row
    ``t * n_streams + s`` = step t of stream s. ``step`` only enqueues kernels on the current stream (no
    allocation in the library, no host sync), so it can follow ``Engine.decode`` and be captured in a HIP graph."""

    def __init__(self, engine: 'Engine', n_streams: int, metric: str = 'l2', n_ori: float = 0.8,
                 alpha_ori: float = 16.49, n_pos: float = 0.5, alpha_pos: float = 48.64):
        self.engine = engine
        self.lib = engine.lib
        self.device = engine.device
        self.n_streams = int(n_streams)
        self.metric = metric.lower()
        h = C.c_void_p()
        L.check(self.lib.spef_video_create(engine.ctx, self.n_streams, L.METRIC_IDS.get(self.metric, -1), n_ori,
                                           alpha_ori, n_pos, alpha_pos, C.byref(h)))
        self.handle = h
        self.last_event = None   # StreamPipeline: the event after the last step it enqueued (steps serialise)

    def step(self, dec: dict, T: int, engine: Optional['Engine'] = None, want_filtered: bool = True) -> dict:
        """``dec``: what ``Engine.decode(..., want_soft=True)`` returned for ``T * n_streams`` time-major frames.
        -> {'ori', 'pos', 'ori_soft', 'pos_soft', 'ori_distance', 'pos_distance', 'status'} of the filtered frames
        (device tensors). ``dec['ori']`` (the still quaternions) gets the pole rule in place. ``engine``: the
        context whose decode tables are used (default: the one the filter was made from; ``StreamPipeline`` passes
        the slot's)."""
        eng = engine or self.engine
        ori_soft, pos_soft, still = dec['ori_soft'], dec['pos_soft'], dec['ori']
        assert ori_soft is not None and pos_soft is not None, 'the video filter needs both soft outputs'
        B, S = ori_soft.shape[0], self.n_streams
        assert T >= 1 and B == T * S, f'{B} frames are not T = {T} steps of {S} streams'
        assert pos_soft.shape[0] == B and still.shape == (B, 4)
        for t in (ori_soft, pos_soft, still):
            assert t.device == self.device and t.is_contiguous() and t.dtype == torch.float32
        dev = self.device
        of = torch.empty_like(ori_soft) if want_filtered else None
        pf = torch.empty_like(pos_soft) if want_filtered else None
        od = torch.empty((B,), dtype=torch.float32, device=dev)
        pd = torch.empty((B,), dtype=torch.float32, device=dev)
        quat = torch.empty((B, 4), dtype=torch.float32, device=dev)
        pos = torch.empty((B, 3), dtype=torch.float32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        L.check(self.lib.spef_video_step(eng.ctx, self.handle, _ptr(ori_soft), _ptr(pos_soft), T, S, _ptr(still),
                                         _ptr(of), _ptr(od), _ptr(pf), _ptr(pd), _ptr(quat), _ptr(pos), _ptr(status),
                                         _stream(dev)))
        return {'ori': quat, 'pos': pos, 'ori_soft': of, 'pos_soft': pf, 'ori_distance': od, 'pos_distance': pd,
                'status': status}

    def reset(self, stream: Optional[int] = None) -> None:
        """Forget one stream's previous PDFs and poles (all streams: None); enqueued on the current stream."""
        L.check(self.lib.spef_video_reset(self.handle, -1 if stream is None else int(stream), _stream(self.device)))

    def set_state(self, stream: int, ori_pdf=None, pos_pdf=None, still_pole=None, video_pole=None) -> None:
        """Load one stream's state (NumPy arrays or tensors; None resets that part)."""
        ts = [None if a is None else torch.as_tensor(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a,
                                                                 np.float32)).to(self.device).contiguous()
              for a in (ori_pdf, pos_pdf, still_pole, video_pole)]
        ob, pg = self.engine._decode_tables
        for t, want in zip(ts, (ob.shape[0], pg.shape[0], 4, 4)):
            assert t is None or t.numel() == want, f'state row of {t.numel()} values, expected {want}'
        L.check(self.lib.spef_video_set_state(self.handle, int(stream), *[_ptr(t) for t in ts], _stream(self.device)))
        for t in ts:
            if t is not None:
                t.record_stream(torch.cuda.current_stream(self.device))

    def close(self) -> None:
        if getattr(self, 'handle', None):
            torch.cuda.synchronize(self.device)
            self.lib.spef_video_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PoseScorer:
    """Device-side pose scoring and evaluation statistics (``Engine.scorer``; csrc/k_score.hip, the arithmetic is
    stated in ``spef_amd.score``): one log of ``capacity`` rows per (group, track).

    Rows are time-major like the video path's: a batch of ``T * n_groups`` rows holds T rows of every group, row
    ``t * n_groups + g`` belongs to group g. ``step`` only enqueues kernels on the current stream (no allocation in
    the library, no host sync): it can follow ``Engine.decode`` / ``VideoFilter.step`` and be captured in a HIP graph.
    ``result`` is the one place that synchronises."""

    def __init__(self, engine: 'Engine', n_groups: int = 1, n_tracks: int = 1, capacity: int = 1 << 16):
        from . import score as SC
        self.engine = engine
        self.lib = engine.lib
        self.device = engine.device
        self.n_groups, self.n_tracks, self.capacity = int(n_groups), int(n_tracks), int(capacity)
        self.fields = SC.STAT_FIELDS
        h = C.c_void_p()
        L.check(self.lib.spef_score_create(engine.ctx, self.n_groups, self.n_tracks, self.capacity, C.byref(h)))
        self.handle = h
        self.last_event = None   # StreamPipeline: the event after the last step it enqueued (steps serialise)

    def _dev(self, a, width: int) -> torch.Tensor:
        """A float32 [rows, width] device tensor of ``a`` (device tensors are used as they are; host arrays are
        copied on the current stream, which then owns the copy)."""
        if isinstance(a, torch.Tensor):
            t = a if a.dtype == torch.float32 else a.float()
        else:
            t = torch.from_numpy(np.array(a, dtype=np.float32, order='C'))   # a copy: read-only arrays are welcome
        return t.to(self.device, non_blocking=True).reshape(-1, width).contiguous()

    def targets(self, targets):
        """``targets`` ({'ori', 'pos'} or a (quat, pos) pair; tensors or arrays) -> the device pair ``step`` takes."""
        q, p = (targets['ori'], targets['pos']) if isinstance(targets, dict) else targets
        return self._dev(q, 4), self._dev(p, 3)

    def step(self, track: int, dec, targets, T: Optional[int] = None, want_rows: bool = False):
        """Score one batch into the logs of ``track``. ``dec``: a decode dict ('ori', 'pos' and, when present,
        'status') or a (quat, pos) pair; ``targets``: as ``targets()``. ``T``: time steps in the batch (default
        rows / n_groups). -> the rows [T * n_groups, 5] (``score.ROW_FIELDS``) as a device tensor when ``want_rows``."""
        if isinstance(dec, dict):
            quat, pos, status = dec['ori'], dec['pos'], dec.get('status')
        else:
            (quat, pos), status = dec, None
        quat, pos = self._dev(quat, 4), self._dev(pos, 3)
        qt, pt = self.targets(targets)
        B, S = quat.shape[0], self.n_groups
        if T is None:
            T = B // S
        assert pos.shape[0] == B and qt.shape[0] == B and pt.shape[0] == B, 'poses and targets differ in rows'
        assert B == T * S, f'{B} rows are not T = {T} steps of {S} groups'
        if status is not None:
            assert status.device == self.device and status.dtype == torch.int32 and status.numel() == B
            status = status.contiguous()
        rows = torch.empty((B, 5), dtype=torch.float32, device=self.device) if want_rows else None
        L.check(self.lib.spef_score_step(self.handle, int(track), _ptr(quat), _ptr(pos), _ptr(status), _ptr(qt),
                                         _ptr(pt), T, S, _ptr(rows), _stream(self.device)))
        return rows

    def reset(self, group: Optional[int] = None) -> None:
        """Empty the logs of one group (all groups: None); enqueued on the current stream."""
        L.check(self.lib.spef_score_reset(self.handle, -1 if group is None else int(group), _stream(self.device)))

    def result(self) -> dict:
        """Run the statistics kernel and synchronise once -> {field: float64 array [n_groups, n_tracks]} for the
        fields of ``score.STAT_FIELDS`` (with no good row every statistic is NaN)."""
        cur = torch.cuda.current_stream(self.device)
        if self.last_event is not None:
            cur.wait_event(self.last_event)
        stats = torch.empty((self.n_groups, self.n_tracks, len(self.fields)), dtype=torch.float64, device=self.device)
        L.check(self.lib.spef_score_finalize(self.handle, _ptr(stats), _stream(self.device)))
        host = stats.cpu().numpy()
        return {k: host[:, :, i].copy() for i, k in enumerate(self.fields)}

    def log(self, track: int = 0, group: int = 0, first: int = 0, n: Optional[int] = None):
        """Slots [first, first + n) of one log -> (rows float32 [n, 5], flags int32 [n]) NumPy arrays
        (synchronises). ``n`` defaults to the capacity's remainder; slots past the log's count hold stale data."""
        n = self.capacity - first if n is None else int(n)
        rows = torch.empty((n, 5), dtype=torch.float32, device=self.device)
        flags = torch.empty((n,), dtype=torch.int32, device=self.device)
        L.check(self.lib.spef_score_log(self.handle, int(track), int(group), int(first), n, _ptr(rows), _ptr(flags),
                                        _stream(self.device)))
        return rows.cpu().numpy(), flags.cpu().numpy()

    def close(self) -> None:
        if getattr(self, 'handle', None):
            torch.cuda.synchronize(self.device)
            self.lib.spef_score_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PoseTracker:
    """Device state of the pose tracker for ``n_streams`` video streams (``Engine.tracker``; csrc/k_track.hip, every
    step is stated in ``spef_amd.spe.track``): an error-state Kalman filter over the per-frame pose of any head, with
    Mahalanobis gating and coasting over frames whose decode failed.

    Rows are time-major like the video path's: a batch of ``T * n_streams`` rows holds T consecutive time steps of
    every stream, row ``t * n_streams + s`` = step t of stream s. ``step`` only enqueues one kernel on the current
    stream (no allocation in the library, no host sync), so it can follow ``Engine.decode`` /
    ``Engine.decode_keypoints`` and be captured in a HIP graph.

    Parameters (``spe.track.DEFAULTS``): ``q`` / ``p0`` process and initial variances of the (theta, t, w, v) blocks,
    ``r`` the fixed measurement variances (theta, t), ``cov_scale``, ``gate_chi2`` (0 = no gate), ``max_coast``. The
    defaults are the constants of the reference's position filter (q = p0 = 1, r = 100; kalman.py), not tuned values:
    a deployment sets them for its own frame rate and noise."""

    def __init__(self, engine: 'Engine', n_streams: int, **params):
        from .spe import track as TK
        self.engine = engine
        self.lib = engine.lib
        self.device = engine.device
        self.n_streams = int(n_streams)
        q, p0, r, cov_scale, gate_chi2, max_coast = TK.check_params(**params)
        self.params = dict(q=tuple(q), p0=tuple(p0), r=tuple(r), cov_scale=cov_scale, gate_chi2=gate_chi2,
                           max_coast=max_coast)
        prm = L.TrackParams((C.c_double * 4)(*q), (C.c_double * 4)(*p0), (C.c_double * 2)(*r), cov_scale, gate_chi2,
                            max_coast)
        h = C.c_void_p()
        L.check(self.lib.spef_track_create(engine.ctx, self.n_streams, C.byref(prm), C.byref(h)))
        self.handle = h
        self.last_event = None   # StreamPipeline: the event after the last step it enqueued (steps serialise)

    def history(self, capacity: int) -> 'PoseHistory':
        """A device buffer for the posteriors of up to ``capacity`` frames of every stream: what ``step(...,
        history=h)`` / ``PoseHistory.push`` record and ``PoseHistory.smooth`` runs the backward pass over."""
        return PoseHistory(self, capacity)

    def step(self, dec: dict, T: int, engine: Optional['Engine'] = None, want_cov: bool = False,
             want_rates: bool = False, history: Optional['PoseHistory'] = None) -> dict:
        """``dec``: a decode dict of ``T * n_streams`` time-major rows: 'ori', 'pos', and when present 'status' (the
        decode status: rows with any of bits 1 | 2 | 4 | 8 are coasted over) and 'cov' ([B x 6 x 6], the pose
        covariance of ``decode_keypoints(want_cov=True)`` or of ``decode_cov``). -> {'ori', 'pos', 'mahalanobis', 'track_status'} and, when
        asked for, 'cov' [B x 6 x 6] (the pose block of P) and 'rates' [B x 6] (w, v) -- device tensors; the inputs are
        left as they are. ``engine`` is accepted for symmetry with ``VideoFilter.step``; the tracker needs no
        tables. With ``history`` (``self.history(capacity)``) the T frames are also recorded for
        ``PoseHistory.smooth``; outputs and state are the same bit for bit."""
        quat, pos, status, cov = dec['ori'], dec['pos'], dec.get('status'), dec.get('cov')
        B, S, dev = quat.shape[0], self.n_streams, self.device
        assert T >= 1 and B == T * S, f'{B} rows are not T = {T} steps of {S} streams'
        assert quat.shape == (B, 4) and pos.shape == (B, 3)
        for t in (quat, pos):
            assert t.device == dev and t.is_contiguous() and t.dtype == torch.float32
        if status is not None:
            assert status.device == dev and status.dtype == torch.int32 and status.numel() == B
            status = status.contiguous()
        if cov is not None:
            assert cov.device == dev and cov.dtype == torch.float32 and cov.numel() == B * 36 and cov.is_contiguous()
        qo = torch.empty((B, 4), dtype=torch.float32, device=dev)
        po = torch.empty((B, 3), dtype=torch.float32, device=dev)
        d2 = torch.empty((B,), dtype=torch.float32, device=dev)
        ts = torch.empty((B,), dtype=torch.int32, device=dev)
        co = torch.empty((B, 6, 6), dtype=torch.float32, device=dev) if want_cov else None
        ro = torch.empty((B, 6), dtype=torch.float32, device=dev) if want_rates else None
        if history is None:
            L.check(self.lib.spef_track_step(self.handle, _ptr(quat), _ptr(pos), _ptr(cov), _ptr(status), T, S,
                                             _ptr(qo), _ptr(po), _ptr(d2), _ptr(co), _ptr(ro), _ptr(ts), _stream(dev)))
        else:   # the same step, bit for bit, with the posterior of every frame appended to ``history``
            assert history.tracker is self, 'the history belongs to another tracker'
            L.check(self.lib.spef_track_step_hist(self.handle, history.handle, _ptr(quat), _ptr(pos), _ptr(cov),
                                                  _ptr(status), T, S, _ptr(qo), _ptr(po), _ptr(d2), _ptr(co),
                                                  _ptr(ro), _ptr(ts), _stream(dev)))
            history.count += T
        out = {'ori': qo, 'pos': po, 'mahalanobis': d2, 'track_status': ts}
        if want_cov:
            out['cov'] = co
        if want_rates:
            out['rates'] = ro
        return out

    def step_modes(self, dec: dict, T: int, want_cov: bool = False, want_rates: bool = False) -> dict:
        """``step`` with several orientation candidates per row: ``dec`` holds ``Engine.decode_modes``' 'mode_quat'
        [B x K x 4], 'mode_mass' [B x K], 'mode_cov' [B x K x 3 x 3] and 'n_modes' [B] next to 'pos', 'cov' (required:
        ``decode_cov``'s, which supplies the t block) and, when present, 'status'. The tracker takes, per row, the
        candidate its prediction makes most likely (the heaviest valid one while the stream has no track; the rule is
        stated in ``spe.track.PoseTrackerHost.step_modes``) and then steps as ``step`` does. -> ``step``'s dict and
        'chosen' [B] int32 (the candidate taken, -1: none). One kernel on the current stream."""
        mq, mm, mc, nm = dec['mode_quat'], dec['mode_mass'], dec['mode_cov'], dec['n_modes']
        pos, status, cov = dec['pos'], dec.get('status'), dec.get('cov')
        B, S, dev = mq.shape[0], self.n_streams, self.device
        K = mq.shape[1]
        assert T >= 1 and B == T * S, f'{B} rows are not T = {T} steps of {S} streams'
        assert cov is not None, 'step_modes needs the pose covariance (decode_cov)'
        assert 1 <= K <= L.MODES_MAX and mq.shape == (B, K, 4) and mm.shape == (B, K) and mc.numel() == B * K * 9
        assert pos.shape == (B, 3) and cov.numel() == B * 36 and nm.numel() == B
        for t in (mq, mm, mc, pos, cov):
            assert t.device == dev and t.is_contiguous() and t.dtype == torch.float32
        assert nm.device == dev and nm.dtype == torch.int32 and nm.is_contiguous()
        if status is not None:
            assert status.device == dev and status.dtype == torch.int32 and status.numel() == B
            status = status.contiguous()
        qo = torch.empty((B, 4), dtype=torch.float32, device=dev)
        po = torch.empty((B, 3), dtype=torch.float32, device=dev)
        d2 = torch.empty((B,), dtype=torch.float32, device=dev)
        ts = torch.empty((B,), dtype=torch.int32, device=dev)
        ch = torch.empty((B,), dtype=torch.int32, device=dev)
        co = torch.empty((B, 6, 6), dtype=torch.float32, device=dev) if want_cov else None
        ro = torch.empty((B, 6), dtype=torch.float32, device=dev) if want_rates else None
        L.check(self.lib.spef_track_step_modes(self.handle, _ptr(mq), _ptr(mm), _ptr(mc), _ptr(nm), K, _ptr(pos),
                                               _ptr(cov), _ptr(status), T, S, _ptr(qo), _ptr(po), _ptr(d2), _ptr(co),
                                               _ptr(ro), _ptr(ts), _ptr(ch), _stream(dev)))
        out = {'ori': qo, 'pos': po, 'mahalanobis': d2, 'track_status': ts, 'chosen': ch}
        if want_cov:
            out['cov'] = co
        if want_rates:
            out['rates'] = ro
        return out

    def predict(self, first: int = 0, n: Optional[int] = None) -> dict:
        """The one-frame-ahead pose of streams [first, first + n) (``spe.roi.predict``): {'ori' [n x 4], 'pos' [n x 3]
        float32: q+ = exp([w]x) q, t+ = t + v; 'have' [n] int32: 0 where the stream has no track (zero pose)}. The
        state is only read; one kernel on the current stream, no host sync."""
        n = self.n_streams - first if n is None else int(n)
        dev = self.device
        qo = torch.empty((max(n, 0), 4), dtype=torch.float32, device=dev)
        po = torch.empty((max(n, 0), 3), dtype=torch.float32, device=dev)
        hv = torch.empty((max(n, 0),), dtype=torch.int32, device=dev)
        L.check(self.lib.spef_track_predict(self.handle, int(first), n, _ptr(qo), _ptr(po), _ptr(hv), _stream(dev)))
        return {'ori': qo, 'pos': po, 'have': hv}

    def reset(self, stream: Optional[int] = None) -> None:
        """Forget one stream's track (all streams: None); enqueued on the current stream."""
        L.check(self.lib.spef_track_reset(self.handle, -1 if stream is None else int(stream), _stream(self.device)))

    def state(self, first: int = 0, n: Optional[int] = None) -> torch.Tensor:
        """The state of streams [first, first + n) as a float64 device tensor [n, 160]: have, consecutive coasted
        frames, 0, q[4], t[3], w[3], v[3], P[144] row-major (enqueued on the current stream)."""
        n = self.n_streams - first if n is None else int(n)
        out = torch.empty((max(n, 0), L.TRACK_STATE_DOUBLES), dtype=torch.float64, device=self.device)
        L.check(self.lib.spef_track_get_state(self.handle, int(first), n, _ptr(out), _stream(self.device)))
        return out

    def set_state(self, state, first: int = 0) -> None:
        """Load the state of streams [first, first + rows) from what ``state`` returned (tensor or array)."""
        if not isinstance(state, torch.Tensor):
            state = torch.from_numpy(np.array(state, dtype=np.float64, order='C'))
        st = state.to(self.device, torch.float64).reshape(-1, L.TRACK_STATE_DOUBLES).contiguous()
        L.check(self.lib.spef_track_set_state(self.handle, int(first), st.shape[0], _ptr(st), _stream(self.device)))
        st.record_stream(torch.cuda.current_stream(self.device))

    def close(self) -> None:
        if getattr(self, 'handle', None):
            torch.cuda.synchronize(self.device)
            self.lib.spef_track_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PoseHistory:
    """The posteriors of up to ``capacity`` frames of every stream of a ``PoseTracker`` on the device
    (``PoseTracker.history``), and the fixed-interval smoother over them (csrc/k_smooth.hip; every step is stated in
    ``spef_amd.spe.smooth``): a Rauch-Tung-Striebel backward pass, so that a recorded video's frame k is estimated
    from every frame of the window. Frames are recorded by ``PoseTracker.step(..., history=self)`` or, after
    ``step_modes`` or live T = 1 steps, by ``push``. ``count`` is the number of frames recorded (kept on the host).
    Nothing here allocates in the library or synchronises after creation."""

    def __init__(self, tracker: PoseTracker, capacity: int):
        self.tracker = tracker
        self.lib = tracker.lib
        self.device = tracker.device
        self.n_streams = tracker.n_streams
        self.capacity = int(capacity)
        self.count = 0
        h = C.c_void_p()
        L.check(self.lib.spef_track_history_create(tracker.handle, self.capacity, C.byref(h)))
        self.handle = h

    def reset(self) -> None:
        """Forget every recorded frame."""
        L.check(self.lib.spef_track_history_reset(self.handle))
        self.count = 0

    def push(self, track_status: torch.Tensor) -> None:
        """Append the tracker's current state as one more frame; ``track_status`` [n_streams] int32 is the
        'track_status' of the step that produced it (one copy kernel on the current stream)."""
        assert track_status.device == self.device and track_status.dtype == torch.int32
        assert track_status.numel() == self.n_streams and track_status.is_contiguous()
        L.check(self.lib.spef_track_history_push(self.handle, self.tracker.handle, _ptr(track_status),
                                                 _stream(self.device)))
        self.count += 1

    def device_count(self) -> torch.Tensor:
        """The number of frames recorded as a device int32 scalar (enqueued on the current stream)."""
        out = torch.empty((), dtype=torch.int32, device=self.device)
        L.check(self.lib.spef_track_history_count(self.handle, _ptr(out), _stream(self.device)))
        return out

    def smooth(self, out: dict, first: int = 0, T: Optional[int] = None, want_cov: bool = False,
               want_rates: bool = False) -> dict:
        """``out``: the tracker's outputs ('ori', 'pos') for the ``T * n_streams`` time-major rows of frames
        ``first .. first + T - 1`` (``T`` None: every frame recorded from ``first`` on). -> {'ori', 'pos',
        'smooth_status'} and, when asked for, 'cov' [B x 6 x 6] (the pose block of P^s) and 'rates' [B x 6] -- new device
        tensors; ``out`` is left as it is. 'smooth_status': 0 smoothed, 1 no track (the row is ``out``'s, 'cov' and
        'rates' NaN), 2 a chain ends here and the row is the filter's (with 4: P- had no Cholesky factor). Two kernels
        on the current stream; without ``want_cov`` no covariance is smoothed."""
        T = self.count - int(first) if T is None else int(T)
        B, dev = T * self.n_streams, self.device
        quat, pos = out['ori'], out['pos']
        assert T >= 1 and quat.shape == (B, 4) and pos.shape == (B, 3), f'{tuple(quat.shape)} is not T = {T} frames'
        for t in (quat, pos):
            assert t.device == dev and t.dtype == torch.float32
        qo, po = quat.clone(memory_format=torch.contiguous_format), pos.clone(memory_format=torch.contiguous_format)
        ss = torch.empty((B,), dtype=torch.int32, device=dev)
        co = torch.empty((B, 6, 6), dtype=torch.float32, device=dev) if want_cov else None
        ro = torch.empty((B, 6), dtype=torch.float32, device=dev) if want_rates else None
        L.check(self.lib.spef_track_smooth(self.handle, int(first), T, _ptr(qo), _ptr(po), _ptr(co), _ptr(ro), _ptr(ss),
                                           _stream(dev)))
        res = {'ori': qo, 'pos': po, 'smooth_status': ss}
        if want_cov:
            res['cov'] = co
        if want_rates:
            res['rates'] = ro
        return res

    def rows(self, first: int = 0, T: Optional[int] = None) -> torch.Tensor:
        """The recorded rows of frames ``first .. first + T - 1`` as a float64 device tensor [T, n_streams, 160]: the
        tracker's state after each frame (``PoseTracker.state``'s layout) with the frame's track status in slot 2."""
        T = self.count - int(first) if T is None else int(T)
        out = torch.empty((max(T, 0), self.n_streams, L.TRACK_STATE_DOUBLES), dtype=torch.float64, device=self.device)
        L.check(self.lib.spef_track_history_get(self.handle, int(first), T, _ptr(out), _stream(self.device)))
        return out

    def close(self) -> None:
        if getattr(self, 'handle', None):
            torch.cuda.synchronize(self.device)
            self.lib.spef_track_history_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ActivationObserver:
    """Histogram observers behind every activation-quantizer input of the float model (``Engine.observer``;
    csrc/k_observe.hip, the statistic is stated in ``spef_amd.quant.observe_host``): one record of 8 counters and
    ``n_bins`` bins per tap, kept on the device and accumulated over every ``observe`` / ``update`` until ``reset``.

    ``observe`` and ``update`` only enqueue kernels on the current stream (no allocation in the library, no host
    sync) and can be captured in a HIP graph; ``read`` is the one place that synchronises."""

    def __init__(self, engine: 'Engine'):
        self.engine = engine
        self.lib = engine.lib
        self.device = engine.device
        h = C.c_void_p()
        L.check(self.lib.spef_observer_create(engine.ctx, C.byref(h)))
        self.handle = h
        nt, nb = C.c_int(), C.c_int()
        L.check(self.lib.spef_observer_info(h, C.byref(nt), C.byref(nb)))
        self.n_taps, self.n_bins = nt.value, nb.value

    def observe(self, frames: torch.Tensor, features: Optional[torch.Tensor] = None) -> None:
        """Run the fp32 schedule on ``frames`` (either layout of ``Engine.forward``) with every tap observed. The
        engine must hold an fp32 blob. ``features`` (optional, the shape ``Engine.backbone`` returns) receives the
        backbone output, bit-identical to ``Engine.backbone``'s."""
        eng = self.engine
        assert frames.device == self.device and frames.is_contiguous()
        layout, B, H, W = eng._layout(frames)
        eng.reserve(B, H, W)
        if features is not None:
            assert features.device == self.device and features.is_contiguous() and features.dtype == torch.float32
        L.check(self.lib.spef_observe(eng.ctx, self.handle, _ptr(frames), layout, B, H, W, _ptr(features),
                                      _stream(self.device)))

    def update(self, tap: int, tensor: torch.Tensor) -> None:
        """Add the values of a float32 device tensor to one tap."""
        assert tensor.device == self.device and tensor.dtype == torch.float32 and tensor.is_contiguous()
        L.check(self.lib.spef_observer_update(self.handle, int(tap), _ptr(tensor), tensor.numel(),
                                              _stream(self.device)))

    def reset(self) -> None:
        """Zero every record; enqueued on the current stream."""
        L.check(self.lib.spef_observer_reset(self.handle, _stream(self.device)))

    def read(self):
        """-> (counters uint64 [taps, 8] = n_total, n_under, n_over, n_nonfinite, max_bits, 0, 0, 0; hist uint64
        [taps, n_bins]) as NumPy arrays (synchronises)."""
        rec = torch.empty((self.n_taps, 8 + self.n_bins), dtype=torch.int64, device=self.device)
        L.check(self.lib.spef_observer_read(self.handle, 0, self.n_taps, _ptr(rec), _stream(self.device)))
        host = rec.cpu().numpy().view(np.uint64)
        return host[:, :8].copy(), host[:, 8:].copy()

    def close(self) -> None:
        if getattr(self, 'handle', None):
            torch.cuda.synchronize(self.device)
            self.lib.spef_observer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HeadTrainer:
    """Device state of a head fit (``Engine.head_trainer``; csrc/k_headfit.hip, every step is stated in
    ``spef_amd.solver.head_fit``): the URSONet head's two Linear layers, their optimizer state and a step counter, trained
    on cached backbone features (``Engine.features``) against soft targets (``Engine.encode_targets``).

    ``step`` and ``evaluate`` only enqueue kernels on the current stream (no allocation in the library, no host sync, no
    atomics) and can be captured in a HIP graph: the learning rate is read from the device tensor ``self.lr`` when the
    update kernel runs and the step counter lives on the device, so every replay is one step further at the rate
    ``set_lr`` last wrote.

    Parameters: ``optimizer`` 'sgd' (torch.optim.SGD with ``momentum``) or 'adam' (torch.optim.Adam with ``beta1``,
    ``beta2``, ``eps``), both with L2 ``weight_decay``; ``pos_mode`` 'classification' or 'regression'; ``beta`` and
    ``norm_distance`` of the reference's SPELoss; ``dropout_p`` on the orientation branch's input (0 = off) with ``seed``;
    ``Bmax`` the largest batch of a step; ``lr`` the initial learning rate."""

    def __init__(self, engine: 'Engine', K: int, n_ori: int, n_pos: int, optimizer: str = 'sgd',
                 pos_mode: str = 'classification', beta: float = 1.0, norm_distance: bool = False,
                 momentum: float = 0.9, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                 weight_decay: float = 0.0, dropout_p: float = 0.0, seed: int = 0, Bmax: int = 64, lr: float = 0.01,
                 ori_mode: str = 'classification'):
        self.engine = engine
        self.lib = engine.lib
        self.device = engine.device
        self.K, self.n_ori, self.n_pos, self.Bmax = int(K), int(n_ori), int(n_pos), int(Bmax)
        self.optimizer, self.pos_mode = optimizer, pos_mode
        modes = {'regression': L.REGRESSION, 'classification': L.CLASSIFICATION}
        assert optimizer in ('sgd', 'adam'), "optimizer must be 'sgd' or 'adam'"
        assert ori_mode in modes and pos_mode in modes, 'modes are regression or classification'
        prm = L.HeadFitParams(modes[ori_mode], modes[pos_mode], L.HEADFIT_ADAM if optimizer == 'adam' else L.HEADFIT_SGD,
                              int(bool(norm_distance)), self.Bmax, int(seed) & 0xFFFFFFFF, float(beta), float(momentum),
                              float(beta1), float(beta2), float(eps), float(weight_decay), float(dropout_p))
        h = C.c_void_p()
        L.check(self.lib.spef_headfit_create(engine.ctx, self.K, self.n_ori, self.n_pos, C.byref(prm), C.byref(h)))
        self.handle = h
        self.lr = torch.full((1,), float(lr), dtype=torch.float32, device=self.device)

    def set_lr(self, lr: float) -> None:
        """Write the learning rate the next steps (and replays of captured ones) read; enqueued."""
        self.lr.fill_(float(lr))

    def _check(self, X, ori_target, pos_target):
        B = X.shape[0]
        for t, w in ((X, self.K), (ori_target, self.n_ori), (pos_target, self.n_pos)):
            assert t.device == self.device and t.dtype == torch.float32 and t.is_contiguous()
            assert tuple(t.shape) == (B, w), f'expected {B} x {w}, got {tuple(t.shape)}'
        return B

    def step(self, X: torch.Tensor, ori_target: torch.Tensor, pos_target: torch.Tensor, want_logits: bool = False,
             want_grad: bool = False, loss: Optional[torch.Tensor] = None) -> dict:
        """One optimisation step on features ``X`` [B x K] with soft targets ``ori_target`` [B x n_ori] and
        ``pos_target`` ([B x n_pos] soft labels, or [B x 3] positions in regression mode). -> {'loss': device float32 [3]
        = total, orientation, position (``loss``, when given, is written and returned), 'logits' [B x (n_ori + n_pos)],
        'grad_w' [Np x K] / 'grad_b' [Np] (dLoss/dW, dLoss/dbias before weight decay; Np = the widths rounded up to 16)}."""
        return self._run(X, ori_target, pos_target, 1, want_logits, want_grad, loss)

    def evaluate(self, X: torch.Tensor, ori_target: torch.Tensor, pos_target: torch.Tensor, want_logits: bool = False,
                 loss: Optional[torch.Tensor] = None) -> dict:
        """The loss (and logits) of a batch without dropout; nothing in the trainer changes."""
        return self._run(X, ori_target, pos_target, 0, want_logits, False, loss)

    def _run(self, X, ori_target, pos_target, train, want_logits, want_grad, loss):
        B = self._check(X, ori_target, pos_target)
        n, Np = self.n_ori + self.n_pos, (self.n_ori + self.n_pos + 15) // 16 * 16
        out = {'loss': loss if loss is not None else torch.empty(3, dtype=torch.float32, device=self.device)}
        if want_logits:
            out['logits'] = torch.empty((B, n), dtype=torch.float32, device=self.device)
        grad = torch.empty(Np * self.K + Np, dtype=torch.float32, device=self.device) if want_grad else None
        L.check(self.lib.spef_headfit_step(self.handle, _ptr(X), _ptr(ori_target), _ptr(pos_target), B, _ptr(self.lr),
                                           train, _ptr(out['loss']), _ptr(out.get('logits')), _ptr(grad),
                                           _stream(self.device)))
        if want_grad:
            out['grad_w'], out['grad_b'] = grad[:Np * self.K].view(Np, self.K), grad[Np * self.K:]
        return out

    def weights(self):
        """-> (W [(n_ori + n_pos) x K], bias [n_ori + n_pos]) device copies; rows = orientation then position."""
        n = self.n_ori + self.n_pos
        W = torch.empty((n, self.K), dtype=torch.float32, device=self.device)
        b = torch.empty(n, dtype=torch.float32, device=self.device)
        L.check(self.lib.spef_headfit_get_weights(self.handle, _ptr(W), _ptr(b), _stream(self.device)))
        return W, b

    def set_weights(self, W, b) -> None:
        n = self.n_ori + self.n_pos
        W = torch.as_tensor(W, dtype=torch.float32).to(self.device).contiguous()
        b = torch.as_tensor(b, dtype=torch.float32).to(self.device).contiguous()
        assert tuple(W.shape) == (n, self.K) and tuple(b.shape) == (n,)
        L.check(self.lib.spef_headfit_set_weights(self.handle, _ptr(W), _ptr(b), _stream(self.device)))

    def state(self):
        """The optimizer state as device copies: SGD -> (buf_W, buf_b); Adam -> (m_W, m_b, v_W, v_b)."""
        n = self.n_ori + self.n_pos
        k = 4 if self.optimizer == 'adam' else 2
        t = [torch.empty((n, self.K) if i % 2 == 0 else (n,), dtype=torch.float32, device=self.device)
             for i in range(k)]
        t += [None] * (4 - k)
        L.check(self.lib.spef_headfit_get_state(self.handle, _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _ptr(t[3]),
                                                _stream(self.device)))
        return tuple(t[:k])

    def last_g(self, B: int) -> torch.Tensor:
        """G = dLoss/dlogits [B x (n_ori + n_pos)] of the last ``step`` / ``evaluate`` of B rows (inspection)."""
        G = torch.empty((B, self.n_ori + self.n_pos), dtype=torch.float32, device=self.device)
        L.check(self.lib.spef_headfit_get_g(self.handle, int(B), _ptr(G), _stream(self.device)))
        return G

    def raw(self, which: str) -> torch.Tensor:
        """One of the trainer's tensors as it lies in memory, padding rows included (inspection): 'W', 'W_s1', 'W_s2'
        [Np x K], 'bias', 'bias_s1', 'bias_s2' [Np] (Np = the widths rounded up to 16; the _s2 tensors under Adam only),
        'Xd' [Bmax x K] (the dropout copy of X the last training step wrote; with dropout on only)."""
        Np = (self.n_ori + self.n_pos + 15) // 16 * 16
        shape = (self.Bmax, self.K) if which == 'Xd' else (Np, self.K) if which.startswith('W') else (Np,)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        L.check(self.lib.spef_headfit_get_raw(self.handle, L.HEADFIT_RAW[which], _ptr(out), _stream(self.device)))
        return out

    def reset_state(self) -> None:
        """Zero the optimizer state and the step counter; enqueued."""
        L.check(self.lib.spef_headfit_reset_state(self.handle, _stream(self.device)))

    def load_model(self) -> None:
        """Copy the engine's head into the trainer (the sizes must be the loaded blob's)."""
        L.check(self.lib.spef_headfit_load_model(self.handle, self.engine.ctx, _stream(self.device)))

    def commit(self) -> None:
        """Copy the trainer's head into the engine: ``Engine.forward`` uses it from the next call on."""
        L.check(self.lib.spef_headfit_commit(self.handle, self.engine.ctx, _stream(self.device)))
        self.engine.epoch += 1

    def close(self) -> None:
        if getattr(self, 'handle', None):
            torch.cuda.synchronize(self.device)
            self.lib.spef_headfit_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """Loaded weights + workspace on one GPU.

    ``forward`` maps NHWC uint8 frames (or the reference's NCHW float32 [0,1] tensor) to the raw head
    outputs; ``decode`` applies SPEUtils.last_activ + decode on the device.
    """

    def __init__(self, blob: bytes | torch.Tensor | None, device: int | str | torch.device = 0):
        """``blob``: packed weights in host memory (bytes) or on this device (uint8 tensor), or None for an empty
        context that receives its weights with ``bcast_weights``."""
        self.lib = L.load()
        self.device = torch.device(device if not isinstance(device, int) else f'cuda:{device}')
        if self.device.type != 'cuda':
            raise AssertionError('SPEMi355x runs on a HIP device only (no CPU fallback)')
        idx = self.device.index or 0
        h = C.c_void_p()
        L.check(self.lib.spef_init(idx, C.byref(h)))
        self.ctx = h
        self._reserved = (0, 0, 0)
        self._decode_tables = None
        self._kp_refine = None      # (max_iters, huber_px) of set_keypoint_refine, or None: off
        self._kp_consensus = None   # (inlier_px, min_inliers or None) of set_keypoint_consensus, or None: off
        # bumped by every call that moves device buffers or changes what a recorded forward / decode would do
        # (workspace reallocation, weights, decode tables, options, camera): StreamPipeline's recorded HIP graphs key on it
        self.epoch = 0
        self.head = self.n_out0 = self.n_out1 = self.n_ops = self.feat_c = None
        self.dtype = None
        self.blob = None
        if blob is not None:
            self.load(blob)

    # ------------------------------------------------------------------ weights
    def load(self, blob: bytes | torch.Tensor) -> None:
        if isinstance(blob, torch.Tensor):
            assert blob.is_cuda and blob.dtype == torch.uint8 and blob.is_contiguous()
            L.check(self.lib.spef_load_weights_device(self.ctx, C.c_void_p(blob.data_ptr()), blob.numel()))
        else:
            buf = C.create_string_buffer(bytes(blob), len(blob))
            L.check(self.lib.spef_load_weights(self.ctx, buf, len(blob)))
        self.blob = blob   # kept so that further contexts (evaluation_device's StreamPipeline) load the same weights
        self._model_info()

    def bcast_weights(self, comm, root: int = 0) -> None:
        """Collective over the RCCL communicator ``comm`` (spef_amd.shard.RcclComm): rank ``root``'s weights are
        broadcast into every rank's context (spef_bcast_weights)."""
        L.check(self.lib.spef_bcast_weights(self.ctx, C.c_void_p(int(comm)), root))
        self._model_info()

    def _model_info(self) -> None:
        head, n0, n1, dt, nops = (C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int())
        L.check(self.lib.spef_model_info(self.ctx, C.byref(head), C.byref(n0), C.byref(n1), C.byref(dt),
                                         C.byref(nops)))
        self.head, self.n_out0, self.n_out1 = head.value, n0.value, n1.value
        self.dtype = {1: 'fp16', 2: 'bf16', 3: 'int8', 4: 'fp32', 5: 'fp16x2', 6: 'fp16mx'}[dt.value]
        self.n_ops = nops.value
        fc = C.c_int()
        L.check(self.lib.spef_feature_width(self.ctx, C.byref(fc)))
        self.feat_c = fc.value   # the width of a `features` row
        self._reserved = (0, 0, 0)
        self.epoch += 1

    def reserve(self, B: int, H: int, W: int) -> None:
        rb, rh, rw = self._reserved
        if B <= rb and (H, W) == (rh, rw):
            return
        L.check(self.lib.spef_reserve(self.ctx, B, H, W))
        self._reserved = (B, H, W)
        self.epoch += 1

    def set_decode_tables(self, ori_bins: Optional[np.ndarray], pos_grid: Optional[np.ndarray]) -> None:
        ob = None if ori_bins is None else np.ascontiguousarray(ori_bins, np.float64)
        pg = None if pos_grid is None else np.ascontiguousarray(pos_grid, np.float64)
        L.check(self.lib.spef_set_decode_tables(
            self.ctx, None if ob is None else ob.ctypes.data_as(C.c_void_p), 0 if ob is None else ob.shape[0],
            None if pg is None else pg.ctypes.data_as(C.c_void_p), 0 if pg is None else pg.shape[0]))
        self._decode_tables = (ob, pg)
        self.epoch += 1

    # ------------------------------------------------------------------ compute
    @staticmethod
    def _layout(x: torch.Tensor) -> Tuple[int, int, int, int]:
        if x.dtype == torch.uint8:
            assert x.dim() == 4 and x.shape[3] == 3, 'uint8 frames must be B x H x W x 3 (NHWC)'
            return L.IN_U8_NHWC, x.shape[0], x.shape[1], x.shape[2]
        assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3, 'expected B x 3 x H x W float32'
        return L.IN_F32_NCHW, x.shape[0], x.shape[2], x.shape[3]

    def forward(self, x: torch.Tensor, out0: Optional[torch.Tensor] = None, out1: Optional[torch.Tensor] = None):
        assert x.device == self.device and x.is_contiguous()
        layout, B, H, W = self._layout(x)
        self.reserve(B, H, W)
        if out0 is None:
            out0 = torch.empty((B, self.n_out0), dtype=torch.float32, device=self.device)
        if out1 is None and self.n_out1:
            out1 = torch.empty((B, self.n_out1), dtype=torch.float32, device=self.device)
        L.check(self.lib.spef_forward(self.ctx, _ptr(x), layout, B, H, W, _ptr(out0), _ptr(out1),
                                      _stream(self.device)))
        return out0, out1

    def preprocess(self, frames: torch.Tensor, size, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decoded frames uint8 [B, Hin, Win, 3] (device) -> uint8 [B, H, W, 3] = Pillow BILINEAR resize
        (transforms.Resize(img_size), speed.py:66-69), ready for ``forward``."""
        assert frames.device == self.device and frames.dtype == torch.uint8 and frames.is_contiguous()
        assert frames.dim() == 4 and frames.shape[3] == 3, 'frames must be B x H x W x 3 uint8'
        B, Hin, Win, _ = frames.shape
        H, W = int(size[0]), int(size[1])
        if out is None:
            out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=self.device)
        L.check(self.lib.spef_preprocess(self.ctx, _ptr(frames), B, Hin, Win, _ptr(out), H, W, _stream(self.device)))
        return out

    def roi_boxes(self, quat: torch.Tensor, pos: torch.Tensor, frame_size, size, margin: float = 0.2,
                  min_side: float = 32.0, have: Optional[torch.Tensor] = None):
        """The box of each pose (``spe.roi.box_of_pose`` states the rule) in frames ``frame_size`` = (Hin, Win) for a
        network input ``size`` = (H, W): -> (box [B x 4] int32 (x0, y0, x1, y1), x1 / y1 exclusive; status [B] int32,
        bit 1 = the row got the full frame). ``have`` [B] int32: ``PoseTracker.predict``'s flag. Needs
        ``set_keypoints``. One kernel on the current stream."""
        dev = self.device
        B = quat.shape[0]
        assert quat.shape == (B, 4) and pos.shape == (B, 3)
        for t in (quat, pos):
            assert t.device == dev and t.is_contiguous() and t.dtype == torch.float32
        if have is not None:
            assert have.device == dev and have.dtype == torch.int32 and have.numel() == B and have.is_contiguous()
        box = torch.empty((B, 4), dtype=torch.int32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        L.check(self.lib.spef_roi_boxes(self.ctx, _ptr(quat), _ptr(pos), _ptr(have), B, int(frame_size[0]),
                                        int(frame_size[1]), int(size[0]), int(size[1]), float(margin), float(min_side),
                                        _ptr(box), _ptr(status), _stream(dev)))
        return box, status

    def preprocess_roi(self, frames: torch.Tensor, boxes: torch.Tensor, size, out: Optional[torch.Tensor] = None,
                       status: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``preprocess`` with one box per frame: frames uint8 [B, Hin, Win, 3], ``boxes`` int32 [B, 4] (device) ->
        uint8 [B, H, W, 3] = Pillow ``crop(box).resize((W, H), BILINEAR)``, bit for bit. ``status`` [B] int32, when
        given, receives 0 or bit 2 (the box is not inside the frame: that frame is zeros)."""
        dev = self.device
        assert frames.device == dev and frames.dtype == torch.uint8 and frames.is_contiguous()
        assert frames.dim() == 4 and frames.shape[3] == 3, 'frames must be B x H x W x 3 uint8'
        B, Hin, Win, _ = frames.shape
        assert boxes.device == dev and boxes.dtype == torch.int32 and boxes.is_contiguous() and boxes.shape == (B, 4)
        if status is not None:
            assert status.device == dev and status.dtype == torch.int32 and status.numel() == B and status.is_contiguous()
        H, W = int(size[0]), int(size[1])
        if out is None:
            out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
        L.check(self.lib.spef_preprocess_roi(self.ctx, _ptr(frames), _ptr(boxes), B, Hin, Win, _ptr(out), H, W,
                                             _ptr(status), _stream(dev)))
        return out

    def unmap_keypoints(self, raw: torch.Tensor, boxes: torch.Tensor, apply_sigmoid: bool = True) -> torch.Tensor:
        """Raw head output of crops [B x 2(n+1)] -> the normalised full-frame keypoints (``spe.roi.unmap``): what
        ``decode_keypoints(apply_sigmoid=False)``, ``consensus_keypoints`` and ``refine_keypoints`` take."""
        dev = self.device
        B = raw.shape[0]
        assert raw.device == dev and raw.dtype == torch.float32 and raw.is_contiguous() and raw.dim() == 2
        assert boxes.device == dev and boxes.dtype == torch.int32 and boxes.is_contiguous() and boxes.shape == (B, 4)
        cfg = getattr(self, '_kp', None)   # without set_keypoints the library refuses (SPEF_ERR_STATE)
        assert cfg is None or raw.shape[1] == 2 * (cfg[0].shape[0] + 1), 'raw must be B x 2(n+1)'
        kp = torch.empty_like(raw)
        L.check(self.lib.spef_roi_unmap_keypoints(self.ctx, _ptr(raw), _ptr(boxes), B, 1 if apply_sigmoid else 0,
                                                  _ptr(kp), _stream(dev)))
        return kp

    def backbone(self, x: torch.Tensor) -> torch.Tensor:
        layout, B, H, W = self._layout(x)
        self.reserve(B, H, W)
        fh, fw = H, W
        for _ in range(5):
            fh, fw = (fh - 1) // 2 + 1, (fw - 1) // 2 + 1
        f = torch.empty((B, fh, fw, 1280), dtype=torch.float32, device=self.device)
        L.check(self.lib.spef_backbone(self.ctx, _ptr(x), layout, B, H, W, _ptr(f), _stream(self.device)))
        return f

    def features(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The pooled backbone features fp32 [B x feat_c] (1280 for MobileNetV2) of frames ``x`` (either layout of
        ``forward``): what ``forward`` hands to the head at the same schedule, bit for bit. URSONet float blobs only."""
        assert x.device == self.device and x.is_contiguous()
        layout, B, H, W = self._layout(x)
        self.reserve(B, H, W)
        if out is None:
            out = torch.empty((B, self.feat_c), dtype=torch.float32, device=self.device)
        assert out.device == self.device and out.dtype == torch.float32 and out.is_contiguous()
        assert out.numel() == B * self.feat_c
        L.check(self.lib.spef_features(self.ctx, _ptr(x), layout, B, H, W, _ptr(out), _stream(self.device)))
        return out

    def encode_targets(self, quat=None, pos=None, ori_var: Optional[float] = None, pos_var: Optional[float] = None,
                       mask=None) -> dict:
        """The reference's soft-classification targets (``OrientationSoftClassification.encode`` /
        ``PositionSoftClassification.encode``) of B poses on this engine's decode tables, on the device. ``quat``
        [B x 4] / ``pos`` [B x 3] (float64; either may be None), ``ori_var`` / ``pos_var`` = (smooth / n_bins_per_dim)^2
        / 12 (defaults: the reference's smooth 3 over 12 bins and 100 over 10), ``mask`` = the redundant-bin flags
        [n_ori]. -> {'ori_soft', 'pos_soft' (float32), 'status' int32 [B x 2]: 1 = that row of that head is NaN}."""
        from .solver import head_fit as HF
        assert quat is not None or pos is not None
        dev = self.device

        def f64(a, w):
            if a is None:
                return None
            if not isinstance(a, torch.Tensor):
                a = torch.from_numpy(np.ascontiguousarray(a, np.float64))
            t = a.to(device=dev, dtype=torch.float64).contiguous()
            assert t.dim() == 2 and t.shape[1] == w
            return t
        q, t = f64(quat, 4), f64(pos, 3)
        B = (q if q is not None else t).shape[0]
        assert t is None or q is None or t.shape[0] == q.shape[0]
        ob, pg = self._decode_tables or (None, None)
        assert (q is None or ob is not None) and (t is None or pg is not None), 'decode table not set'
        out = {'status': torch.empty((B, 2), dtype=torch.int32, device=dev)}
        if q is not None:
            out['ori_soft'] = torch.empty((B, ob.shape[0]), dtype=torch.float32, device=dev)
        if t is not None:
            out['pos_soft'] = torch.empty((B, pg.shape[0]), dtype=torch.float32, device=dev)
        m = None
        if mask is not None:
            m = torch.as_tensor(np.ascontiguousarray(np.asarray(mask), np.uint8)).to(dev)
            assert ob is not None and m.numel() == ob.shape[0]
        prm = L.EncodeParams(HF.soft_variance(3, 12) if ori_var is None else float(ori_var),
                             HF.soft_variance(100, 10) if pos_var is None else float(pos_var))
        L.check(self.lib.spef_encode_targets(self.ctx, _ptr(q), _ptr(t), B, C.byref(prm), _ptr(m),
                                             _ptr(out.get('ori_soft')), _ptr(out.get('pos_soft')), _ptr(out['status']),
                                             _stream(dev)))
        return out   # (q, t, m are stream-ordered temporaries of torch's allocator: the kernel reads them before any reuse)

    def head_trainer(self, K: Optional[int] = None, n_ori: Optional[int] = None, n_pos: Optional[int] = None,
                     **params) -> 'HeadTrainer':
        """A head fit on this engine's device (``HeadTrainer``). Without sizes it takes the loaded URSONet blob's (its
        feature width and its two head widths) and starts from the blob's head; with sizes it is a standalone trainer that starts
        at zero weights."""
        if K is None and n_ori is None and n_pos is None:
            assert self.head == 0, 'no URSONet blob loaded: give K, n_ori, n_pos'
            tr = HeadTrainer(self, self.feat_c, self.n_out0, self.n_out1, **params)
            tr.load_model()
            return tr
        return HeadTrainer(self, K, n_ori, n_pos, **params)

    def probe(self, x: torch.Tensor, stop_op: int) -> torch.Tensor:
        layout, B, H, W = self._layout(x)
        self.reserve(B, H, W)
        out = torch.empty(B * H * W * 96 // 4 + 64, dtype=torch.float32, device=self.device)  # >= any act
        c, h, w = C.c_int(), C.c_int(), C.c_int()
        L.check(self.lib.spef_probe(self.ctx, _ptr(x), layout, B, H, W, stop_op, _ptr(out), C.byref(c), C.byref(h),
                                    C.byref(w), _stream(self.device)))
        return out[:B * h.value * w.value * c.value].view(B, h.value, w.value, c.value)

    def decode(self, ori_mode: int, pos_mode: int, ori_raw: torch.Tensor, pos_raw: torch.Tensor,
               want_soft: bool = True, want_cov: bool = False, **cov_params):
        """``want_cov`` (off by default): ``decode_cov`` follows the decode on the same stream and adds 'cov',
        'cov_status' (and 'ori_hinv' with ``want_hinv=True``) to the dict; it needs the soft outputs, so they are
        returned as well. ``cov_params``: fixed_var, floor_var, want_hinv."""
        assert want_cov or not cov_params, 'fixed_var / floor_var / want_hinv go with want_cov'
        want_soft = want_soft or want_cov
        B = ori_raw.shape[0]
        dev = self.device
        quat = torch.empty((B, 4), dtype=torch.float32, device=dev)
        pos = torch.empty((B, 3), dtype=torch.float32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        ori_soft = torch.empty_like(ori_raw) if (want_soft and ori_mode == L.CLASSIFICATION) else None
        pos_soft = torch.empty_like(pos_raw) if (want_soft and pos_mode == L.CLASSIFICATION) else None
        assert ori_raw.dim() == 2 and pos_raw.dim() == 2 and pos_raw.shape[0] == B
        assert ori_raw.is_contiguous() and pos_raw.is_contiguous()
        assert ori_raw.dtype == torch.float32 and pos_raw.dtype == torch.float32
        L.check(self.lib.spef_decode(self.ctx, ori_mode, pos_mode, _ptr(ori_raw), ori_raw.shape[1], _ptr(pos_raw),
                                     pos_raw.shape[1], B, _ptr(ori_soft), _ptr(quat), _ptr(pos_soft), _ptr(pos),
                                     _ptr(status), _stream(dev)))
        dec = {'ori': quat, 'pos': pos, 'ori_soft': ori_soft, 'pos_soft': pos_soft, 'status': status}
        if want_cov:
            self.decode_cov(dec, ori_mode, pos_mode, **cov_params)
        return dec

    def decode_cov(self, dec: dict, ori_mode: int, pos_mode: int, fixed_var=(100.0, 100.0), floor_var=(0.0, 0.0),
                   want_hinv: bool = False) -> dict:
        """The pose covariance of a soft-classification decode (csrc/k_cov.hip; ``spe.decode_cov`` is its NumPy twin
        and states every quantity): adds 'cov' [B x 6 x 6] -- the measurement covariance ``PoseTracker.step`` reads,
        order (theta, t) -- 'cov_status' [B] (1 theta block NaN, 2 the Markley matrix is not positive definite, 4 t
        block NaN; a word of its own, the decode 'status' is left alone) and, with ``want_hinv``, 'ori_hinv'
        [B x 4 x 4] (the inverse Markley matrix the reference's decode returns and drops) to ``dec`` and returns it.
        ``dec`` is any PDF + pose pair: what ``decode`` returned, or ``VideoFilter.step``'s filtered PDFs with their
        decode. A head in regression mode gets ``fixed_var[k]`` I (pass the tracker's ``r``); ``floor_var`` is added to
        the diagonal of a classification head's block. One launch on the current stream; no host sync."""
        quat, pos = dec['ori'], dec['pos']
        B, dev = quat.shape[0], self.device
        oc, pc = ori_mode == L.CLASSIFICATION, pos_mode == L.CLASSIFICATION
        op, pp = (dec.get('ori_soft') if oc else None), (dec.get('pos_soft') if pc else None)
        assert not oc or op is not None, 'decode_cov needs the orientation PDF (want_soft)'
        assert not pc or pp is not None, 'decode_cov needs the position PDF (want_soft)'
        assert not want_hinv or oc, 'ori_hinv needs the orientation head in classification mode'
        for t in (quat, pos, op, pp):
            assert t is None or (t.device == dev and t.is_contiguous() and t.dtype == torch.float32 and
                                 t.shape[0] == B)
        assert quat.shape == (B, 4) and pos.shape == (B, 3)
        fx, fl = (np.asarray(v, np.float64).reshape(-1) for v in (fixed_var, floor_var))
        assert fx.size == 2 and fl.size == 2, 'fixed_var and floor_var are (theta, t) pairs'
        prm = L.CovParams((C.c_double * 2)(*fx), (C.c_double * 2)(*fl))
        cov = torch.empty((B, 6, 6), dtype=torch.float32, device=dev)
        hinv = torch.empty((B, 4, 4), dtype=torch.float32, device=dev) if want_hinv else None
        cst = torch.empty((B,), dtype=torch.int32, device=dev)
        L.check(self.lib.spef_decode_cov(self.ctx, ori_mode, pos_mode, _ptr(op), op.shape[1] if oc else 0, _ptr(pp),
                                         pp.shape[1] if pc else 0, _ptr(quat), _ptr(pos), B, C.byref(prm), _ptr(cov),
                                         _ptr(hinv), _ptr(cst), _stream(dev)))
        dec['cov'], dec['cov_status'] = cov, cst
        if want_hinv:
            dec['ori_hinv'] = hinv
        return dec

    def decode_modes(self, dec_or_pdf, k_max: int = 2, sep_deg: float = 45.0, seed_rel: float = 0.1,
                     min_mass: float = 0.05, rounds: int = 3, floor_var: float = 0.0) -> dict:
        """The multi-hypothesis orientation decode (csrc/k_modes.hip; ``spe.modes`` is its NumPy twin and states the
        algorithm): up to ``k_max`` orientations that a soft-classification PDF holds at once, where ``decode`` returns
        their one Markley average. ``dec_or_pdf``: an orientation PDF [B x n_ori] (float32, on the device) or a dict
        holding one as 'ori_soft' (what ``decode`` or ``VideoFilter.step`` returned), which then also receives the
        results. -> {'mode_quat' [B x k_max x 4] (unit, scalar part >= 0, by descending mass), 'mode_mass'
        [B x k_max], 'mode_cov' [B x k_max x 3 x 3] (each mode's theta block; ``floor_var`` is added to its diagonal),
        all NaN past 'n_modes' [B], and 'modes_status' [B] (1: the row is not a PDF; a word of its own)}. With one mode
        the result is the plain decode, mass 1 and ``decode_cov``'s theta block. ``PoseTracker.step_modes`` takes the
        dict. One launch on the current stream; no host sync."""
        from .spe import modes as MD
        k_max, rounds, sep_deg, seed_rel, min_mass, floor_var = MD.check_params(k_max, sep_deg, seed_rel, min_mass,
                                                                                rounds, floor_var)
        dec = dec_or_pdf if isinstance(dec_or_pdf, dict) else None
        pdf = dec.get('ori_soft') if dec is not None else dec_or_pdf
        assert pdf is not None, 'decode_modes needs the orientation PDF (want_soft; a classification head)'
        dev = self.device
        assert pdf.dim() == 2 and pdf.device == dev and pdf.is_contiguous() and pdf.dtype == torch.float32
        B = pdf.shape[0]
        prm = L.ModesParams(k_max, rounds, sep_deg, seed_rel, min_mass, floor_var)
        mq = torch.empty((B, k_max, 4), dtype=torch.float32, device=dev)
        mm = torch.empty((B, k_max), dtype=torch.float32, device=dev)
        mc = torch.empty((B, k_max, 3, 3), dtype=torch.float32, device=dev)
        nm = torch.empty((B,), dtype=torch.int32, device=dev)
        ms = torch.empty((B,), dtype=torch.int32, device=dev)
        L.check(self.lib.spef_decode_modes(self.ctx, _ptr(pdf), pdf.shape[1], B, C.byref(prm), _ptr(mq), _ptr(mm),
                                           _ptr(mc), _ptr(nm), _ptr(ms), _stream(dev)))
        out = {'mode_quat': mq, 'mode_mass': mm, 'mode_cov': mc, 'n_modes': nm, 'modes_status': ms}
        if dec is not None:
            dec.update(out)
        return out

    def video_filter(self, n_streams: int, metric: str = 'l2', n_ori: float = 0.8, alpha_ori: float = 16.49,
                     n_pos: float = 0.5, alpha_pos: float = 48.64) -> 'VideoFilter':
        """The adaptive video filter (``TemporalPDF.update_pdf`` + pole continuity) for ``n_streams`` independent
        streams on this engine's device; the defaults are the reference ``Inference`` engine's (inference.py:38-39).
        Needs both decode tables."""
        return VideoFilter(self, n_streams, metric, n_ori, alpha_ori, n_pos, alpha_pos)

    def scorer(self, n_groups: int = 1, n_tracks: int = 1, capacity: int = 1 << 16) -> 'PoseScorer':
        """Device-side scoring (``SPEUtils.get_score``) and evaluation statistics for ``n_groups`` groups of rows
        (videos, cameras; 1 for a plain evaluation) and ``n_tracks`` kinds of pose (still, filtered), with room for
        ``capacity`` rows per (group, track), at most 2^20."""
        return PoseScorer(self, n_groups, n_tracks, capacity)

    def tracker(self, n_streams: int, **params) -> 'PoseTracker':
        """The pose tracker (an error-state Kalman filter with gating and coasting) for ``n_streams`` independent
        video streams on this engine's device; works behind every head. ``params``: q, p0, r, cov_scale, gate_chi2,
        max_coast (``PoseTracker``; the defaults are the reference filter's constants, not tuned)."""
        return PoseTracker(self, n_streams, **params)

    def observer(self) -> 'ActivationObserver':
        """Histogram observers for the INT8 calibration (``quant.calibrate_device``): one tap per activation
        quantizer of the loaded model. ``observe`` needs an fp32 blob in this engine."""
        return ActivationObserver(self)

    def set_fused(self, on: bool) -> None:
        """Fused inverted-residual blocks (default) or one kernel per conv (reference schedule)."""
        L.check(self.lib.spef_set_option(self.ctx, L.OPT_FUSE_BLOCKS, 1 if on else 0))

    def set_option(self, option: int, value: int) -> None:
        L.check(self.lib.spef_set_option(self.ctx, option, int(value)))
        self.epoch += 1

    def set_keypoints(self, kp3d: np.ndarray, K: np.ndarray, nu: float, nv: float, dist=None) -> None:
        """Keypoint-mode camera: 3-D model points, K, image size; ``dist`` = the camera's distCoeffs (k1, k2, p1,
        p2[, k3]; SPEED+) or None (SPEED: cv2.solvePnP gets zeros, keypoints_utils.py:136)."""
        kp = np.ascontiguousarray(kp3d, np.float32)
        kk = np.ascontiguousarray(K, np.float64).reshape(9)
        L.check(self.lib.spef_set_keypoints(self.ctx, kp.ctypes.data_as(C.c_void_p), kp.shape[0],
                                            kk.ctypes.data_as(C.c_void_p), float(nu), float(nv)))
        dd = np.zeros(0) if dist is None else np.ascontiguousarray(np.asarray(dist, np.float64).reshape(-1))
        L.check(self.lib.spef_set_keypoint_distortion(self.ctx, dd.ctypes.data_as(C.c_void_p) if dd.size else None,
                                                      int(dd.size)))
        self.epoch += 1
        self._kp = (kp, kk, dd)

    def decode_keypoints(self, raw: torch.Tensor, apply_sigmoid: bool = True, want_cov: bool = False):
        """``want_cov``: with the refinement on (``set_keypoint_refine``), add 'cov' [B x 6 x 6], the refined pose's
        covariance (what ``PoseTracker.step`` takes as the measurement covariance). Off by default."""
        B = raw.shape[0]
        dev = self.device
        kp = torch.empty_like(raw)
        quat = torch.empty((B, 4), dtype=torch.float32, device=dev)
        pos = torch.empty((B, 3), dtype=torch.float32, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        L.check(self.lib.spef_decode_keypoints(self.ctx, _ptr(raw), B, 1 if apply_sigmoid else 0, _ptr(kp), _ptr(quat),
                                               _ptr(pos), _ptr(status), _stream(dev)))
        dec = {'keypoints': kp, 'ori': quat, 'pos': pos, 'status': status}
        refine, weights, q0, t0 = self._kp_refine, None, quat, pos
        if self._kp_consensus is not None:   # set_keypoint_consensus: inlier selection behind EPnP, same stream
            con = self.consensus_keypoints(kp, quat, pos, inlier_px=self._kp_consensus[0],
                                           min_inliers=self._kp_consensus[1], status=status)
            dec.update(inliers=con['inliers'], n_inliers=con['n_inliers'], ori_consensus=con['ori'],
                       pos_consensus=con['pos'])
            weights, q0, t0 = con['weights'], con['ori'], con['pos']
            if refine is None:               # least squares on the inliers
                refine = (20, 0.0)
        if refine is not None:   # set_keypoint_refine: Levenberg-Marquardt behind EPnP, same stream
            ref = self.refine_keypoints(kp, q0, t0, weights=weights, max_iters=refine[0], huber_px=refine[1],
                                        status=status, want_cov=want_cov)
            dec.update(ori=ref['ori'], pos=ref['pos'], ori_epnp=quat, pos_epnp=pos, fit=ref['fit'],
                       refine_iters=ref['iters'])
            if want_cov:
                dec['cov'] = ref['cov']
        return dec

    def set_keypoint_consensus(self, inlier_px=None, min_inliers=None) -> None:
        """Turn the 3-point consensus between EPnP and the refinement on (``inlier_px``: the inlier threshold in
        pixels; ``min_inliers``: 4..n, None = max(4, ceil(n / 2))) or off (``inlier_px`` 0 or None, the default).
        With it on, ``decode_keypoints`` runs EPnP, the consensus and the refinement kernel on one stream: the
        refinement starts from the consensus pose with the inlier weights, with ``set_keypoint_refine``'s settings
        when that is on and (20 trials, plain least squares) otherwise. The result gains 'inliers' [B x n] bool,
        'n_inliers', 'ori_consensus', 'pos_consensus' and the refinement's keys; a row without consensus carries the
        informational status bit 64 and is EPnP's pose (+ refinement), as with the consensus off."""
        if not inlier_px:
            self._kp_consensus = None
            return
        inlier_px = float(inlier_px)
        assert np.isfinite(inlier_px) and inlier_px > 0, 'inlier_px must be finite and > 0'
        assert min_inliers is None or int(min_inliers) >= 4, 'min_inliers must be in 4..n'
        self._kp_consensus = (inlier_px, None if min_inliers is None else int(min_inliers))

    def consensus_keypoints(self, kp: torch.Tensor, quat: torch.Tensor, pos: torch.Tensor, weights=None,
                            inlier_px: float = 8.0, min_inliers=None, status=None, want_pose64: bool = False) -> dict:
        """Exhaustive 3-point consensus (csrc/k_consensus.hip; ``spe.consensus.consensus_host`` is its NumPy twin)
        on the normalised keypoints ``kp`` [B x 2(n+1)] (after the sigmoid) from the start pose ``quat`` / ``pos``
        (EPnP's), with optional confidences ``weights`` [B x n] (points with 0 are neither sampled nor scored). The
        inputs are left as they are. -> {'ori', 'pos' (the winning hypothesis; the start pose on a row without
        consensus), 'inliers' [B x n] bool, 'weights' [B x n] (the confidences of the inliers, 0 elsewhere: what
        ``refine_keypoints`` takes), 'n_inliers', 'triple', 'root', 'scored' [B] int32, 'cost' [B], 'status'}.
        ``status`` [B] int32, when given, is ORed into in place: bit 64 = no consensus. ``want_pose64`` adds 'R'
        [B x 3 x 3] and 't' [B x 3], the winning hypothesis in float64 as it was scored (NaN without consensus)."""
        B = kp.shape[0]
        dev = self.device
        assert kp.dtype == torch.float32 and kp.is_contiguous() and kp.dim() == 2
        n = kp.shape[1] // 2 - 1
        q = quat.detach().to(dev, torch.float32).reshape(B, 4).clone()
        t = pos.detach().to(dev, torch.float32).reshape(B, 3).clone()
        w = None
        if weights is not None:
            w = weights.detach().to(dev, torch.float32).contiguous()
            assert w.dim() == 2 and w.shape[0] == B and w.shape[1] == n
        if min_inliers is None:
            min_inliers = max(4, (n + 1) // 2)
        wout = torch.empty((B, n), dtype=torch.float32, device=dev)
        info = torch.empty((B, 4), dtype=torch.int32, device=dev)
        cost = torch.empty((B,), dtype=torch.float32, device=dev)
        if status is None:
            status = torch.zeros((B,), dtype=torch.int32, device=dev)
        assert status.dtype == torch.int32 and status.is_contiguous() and status.numel() == B
        p64 = torch.empty((B, 12), dtype=torch.float64, device=dev) if want_pose64 else None
        if want_pose64:
            L.check(self.lib.spef_consensus_keypoints_f64(self.ctx, _ptr(kp), _ptr(w), B, float(inlier_px),
                                                          int(min_inliers), _ptr(q), _ptr(t), _ptr(wout), _ptr(info),
                                                          _ptr(cost), _ptr(p64), _ptr(status), _stream(dev)))
        else:
            L.check(self.lib.spef_consensus_keypoints(self.ctx, _ptr(kp), _ptr(w), B, float(inlier_px),
                                                      int(min_inliers), _ptr(q), _ptr(t), _ptr(wout), _ptr(info),
                                                      _ptr(cost), _ptr(status), _stream(dev)))
        extra = {'R': p64[:, :9].reshape(B, 3, 3), 't': p64[:, 9:]} if want_pose64 else {}
        return {**extra, 'ori': q, 'pos': t, 'inliers': (wout > 0) & (info[:, 1:2] >= 0), 'weights': wout,
                'n_inliers': info[:, 0], 'triple': info[:, 1], 'root': info[:, 2], 'scored': info[:, 3], 'cost': cost,
                'status': status}

    def set_keypoint_refine(self, max_iters=None, huber_px: float = 0.0) -> None:
        """Turn the pose refinement behind EPnP on (``max_iters`` trials in 1..100, Huber threshold ``huber_px`` in
        pixels, 0 = plain least squares) or off (``max_iters`` 0 or None, the default). With it on,
        ``decode_keypoints`` returns the refined 'ori' / 'pos' and adds 'ori_epnp', 'pos_epnp', 'fit' and
        'refine_iters'; 'status' may carry the informational bits 16 (row not refined) and 32 (stopped at
        ``max_iters``)."""
        if not max_iters:
            self._kp_refine = None
            return
        max_iters, huber_px = int(max_iters), float(huber_px)
        assert 1 <= max_iters <= 100, 'max_iters must be in 1..100'
        assert np.isfinite(huber_px) and huber_px >= 0, 'huber_px must be finite and >= 0'
        self._kp_refine = (max_iters, huber_px)

    def refine_keypoints(self, kp: torch.Tensor, quat: torch.Tensor, pos: torch.Tensor, weights=None,
                         max_iters: int = 50, huber_px: float = 0.0, want_cov: bool = False, status=None) -> dict:
        """Robust Levenberg-Marquardt refinement (csrc/k_refine.hip; ``spe.refine.refine_pose_host`` is its NumPy
        twin) of the poses ``quat`` [B x 4] / ``pos`` [B x 3] -- EPnP's, a classification head's, the previous
        frame's -- against the normalised keypoints ``kp`` [B x 2(n+1)] (after the sigmoid), with optional per-point
        confidences ``weights`` [B x n]. The inputs are left as they are. -> {'ori', 'pos', 'fit' [B x 4]: RMS px
        before / after, cost before / after, 'iters', 'status'} and, with ``want_cov``, 'cov' [B x 6 x 6] (order
        omega_xyz, t_xyz). ``status`` [B] int32, when given, is ORed into in place (EPnP's word: a row with bit 8 is
        not refined)."""
        B = kp.shape[0]
        dev = self.device
        assert kp.dtype == torch.float32 and kp.is_contiguous() and kp.dim() == 2
        q = quat.detach().to(dev, torch.float32).reshape(B, 4).clone()
        t = pos.detach().to(dev, torch.float32).reshape(B, 3).clone()
        w = None
        if weights is not None:
            w = weights.detach().to(dev, torch.float32).contiguous()
            assert w.dim() == 2 and w.shape[0] == B and 2 * (w.shape[1] + 1) == kp.shape[1]
        fit = torch.empty((B, 4), dtype=torch.float32, device=dev)
        cov = torch.empty((B, 6, 6), dtype=torch.float32, device=dev) if want_cov else None
        iters = torch.empty((B,), dtype=torch.int32, device=dev)
        if status is None:
            status = torch.zeros((B,), dtype=torch.int32, device=dev)
        assert status.dtype == torch.int32 and status.is_contiguous() and status.numel() == B
        L.check(self.lib.spef_refine_keypoints(self.ctx, _ptr(kp), _ptr(w), B, int(max_iters), float(huber_px),
                                               _ptr(q), _ptr(t), _ptr(fit), _ptr(cov), _ptr(iters), _ptr(status),
                                               _stream(dev)))
        out = {'ori': q, 'pos': t, 'fit': fit, 'iters': iters, 'status': status}
        if want_cov:
            out['cov'] = cov
        return out

    # ------------------------------------------------------------------ profiling
    def profile_begin(self) -> None:
        L.check(self.lib.spef_profile_begin(self.ctx))

    def profile_end(self) -> dict:
        """-> {kernel key: (launches, total_ms, algorithmic_bytes, algorithmic_flops)}."""
        import json
        need = C.c_size_t(0)
        buf = C.create_string_buffer(1 << 16)
        L.check(self.lib.spef_profile_end(self.ctx, buf, len(buf), C.byref(need)))
        return {k: tuple(v) for k, v in json.loads(buf.value.decode()).items()}

    def close(self) -> None:
        if getattr(self, 'ctx', None):
            self.lib.spef_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
