"""Batch engine: device buffers (torch tensors), contexts, and the batched planner over libfcpp.so.

torch is used for device memory and streams only; all arithmetic happens in the HIP library.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib as L

_contexts = {}


def _torch():
    import torch
    return torch


class Context:
    """One fcpp_ctx per device, bound to torch's current stream at every call."""

    def __init__(self, device=0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise RuntimeError('no GPU visible: the fcpp operators have no CPU fallback')
        self.device = int(device)
        self.lib = L.load()
        h = C.c_void_p()
        L.check(self.lib.fcpp_ctx_create(self.device, C.byref(h)))
        self.handle = h
        self._bound = None          # the stream handle the library was last given
        self._arena = None          # (lane, pitch) of the output arena, asked once

    def bind_stream(self):
        torch = _torch()
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._bound:        # (only this method sets the library's stream)
            L.check(self.lib.fcpp_ctx_set_stream(self.handle, C.c_void_p(s)))
            self._bound = s

    def arena(self):
        """-> (lane bytes, pitch bytes) of the output arena, (0, 0) without one; asked once (reserve_outputs asks again)"""
        if self._arena is None:
            self._arena = self.outputs_info()[:2]
        return self._arena

    def direct_steps(self):
        """Direct steps Batch.plan has launched on this context so far (fcpp_ctx_direct_steps): the step enqueued right behind the device
        setup's counting pass, before the totals are back; the batch's tables are then filled when somebody asks for them."""
        return self.direct_counts()[0]

    def direct_counts(self):
        """-> (direct steps launched, calls whose batch was TAKEN -- no fill pass and no run in the call --, fill passes of taken batches
        enqueued since: somebody asked for the tables, or another setup took the plan slot)"""
        n, t, f = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self.lib.fcpp_ctx_direct_steps(self.handle, C.byref(n), C.byref(t), C.byref(f)))
        return n.value, t.value, f.value

    def cut_rows_passes(self):
        """Direct setups on this context so far whose counting pass took its row form (fcpp_ctx_cut_rows_passes); FCPP_CUT_ROWS=0, read
        per call, keeps the form of a wavefront per field: its checker."""
        n = C.c_int64()
        L.check(self.lib.fcpp_ctx_cut_rows_passes(self.handle, C.byref(n)))
        return n.value

    def reserve_outputs(self, lane_gib=24.0, pitch_gib=24.0):
        """Give the context its output ARENA (fcpp_ctx_reserve_outputs): one device allocation of 4 x pitch + lane, made once -- it takes
        the driver seconds, so it belongs to start-up, not to a plan call -- in which Batch.alloc() then places the five output arrays of
        every batch a pitch apart (far apart they are written a class faster than back to back).  Any number of live
        batches share it.  Raises when the device has not that much room."""
        L.check(self.lib.fcpp_ctx_reserve_outputs(self.handle, int(lane_gib * 2**30), int(pitch_gib * 2**30)))
        self._arena = None

    def outputs_info(self):
        """-> (lane bytes, pitch bytes, live bytes per lane) of the output arena; zeros without one"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self.lib.fcpp_ctx_outputs_info(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_setup(self, mode):
        """Where batches are set up from now on: 'auto' (on the device where the device planner takes the batch: the reference's sampling,
        no obstacle-aware swaths), 'host', 'device' (fcpp_ctx_set_setup)."""
        m = {'auto': L.SETUP_AUTO, 'host': L.SETUP_HOST, 'device': L.SETUP_DEVICE}[mode] if isinstance(mode, str) else int(mode)
        L.check(self.lib.fcpp_ctx_set_setup(self.handle, m))

    def __del__(self):
        try:
            if getattr(self, 'handle', None):
                self.lib.fcpp_ctx_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


def get_context(device=None):
    torch = _torch()
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    device = int(device)
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def make_vehicle(vp=None, **kw):
    """fcpp_vehicle from a VehicleParams-like object (attributes named as MLP:31-38) or keywords."""
    v = L.default_vehicle()
    if vp is not None:
        for n, _ in L.Vehicle._fields_:
            setattr(v, n, float(getattr(vp, n)))
    for k, val in kw.items():
        setattr(v, k, float(val))
    return v


def make_options(turn_model=L.TURN_ARC, sample_spacing=0.0, clothoid_frac=0.5, clothoid_fit=1, geofence_tol=1e-6,
                 avoid_obstacles=False, ring_order=L.RING_AS_VERTICES):
    """fcpp_options.  avoid_obstacles: clip the swaths of layer 1 at the obstacles and drive around them (build-defined,
    include/fcpp.h); False = the reference's behaviour (obstacles only flag the points inside them)."""
    o = L.default_options()
    o.obstacle_mode = L.OBSTACLES_AVOID if avoid_obstacles else L.OBSTACLES_FLAG
    o.turn_model = int(turn_model)
    o.sample_spacing = float(sample_spacing)
    o.clothoid_frac = float(clothoid_frac)
    o.clothoid_fit = int(clothoid_fit)
    o.geofence_tol = float(geofence_tol)
    o.ring_order = int(ring_order)      # order of the inset corners in Shapely's buffer(-d).exterior.coords (include/fcpp.h)
    return o


@dataclass
class FieldSpec:
    """Constructor arguments of one planner (MLP:63-72)."""
    field_length: float = None
    field_width: float = None
    field_vertices: list = None
    obstacles: list = None
    start_point: tuple = None
    end_point: tuple = None


_FIELD_DT = None


def _field_dtype():
    global _FIELD_DT
    if _FIELD_DT is None:
        _FIELD_DT = np.dtype(L.Field)          # fcpp_field as a numpy record (same layout as the ctypes structure)
    return _FIELD_DT


class FieldTable:
    """The constructor arguments of n planners as ONE array of fcpp_field records (+ the batch's obstacle polygons in CSR form): what
    fcpp_batch_create / fcpp_plan_count take, built with array operations instead of a Python loop over FieldSpec objects (65 536
    specs cost 0.45 s to build and pack one by one; the table of the same fields 3 ms).

        FieldTable.from_rectangles(LH)            (n, 2) array of (field_length, field_width)                  MLP:127-132
        FieldTable.from_vertices(V)               (n, 4, 2) array of field_vertices                              MLP:116-122
        FieldTable.from_specs([FieldSpec, ...])   the general case (obstacles, start / end points per field)

    start_points / end_points: (n, 2) arrays, NaN rows = not given.  A table can be sliced (`table[lo:hi]`: the shard of a rank); the
    slice shares the polygon table."""

    def __init__(self, rec, poly_offsets=None, poly_x=None, poly_y=None):
        self._cargs = None
        self._dev = None            # the records' copy in device memory after to_device() (a torch uint8 tensor)
        self.rec = rec
        self._pinned = None         # the pinned buffer the records live in after pin()
        self.poly_offsets = np.zeros(1, dtype=np.int64) if poly_offsets is None else np.ascontiguousarray(poly_offsets, dtype=np.int64)
        self.poly_x = np.zeros(0, dtype=np.float64) if poly_x is None else np.ascontiguousarray(poly_x, dtype=np.float64)
        self.poly_y = np.zeros(0, dtype=np.float64) if poly_y is None else np.ascontiguousarray(poly_y, dtype=np.float64)

    @property
    def rec(self):
        """the fcpp_field records (a numpy record array; written in place they stay what the library reads)"""
        return self._rec

    @rec.setter
    def rec(self, value):
        self._rec = value
        self._cargs = None          # (the pointers c_args() made are another array's)
        self._dev = None            # (and so is the copy on the device)

    def __len__(self):
        return int(self.rec.shape[0])

    def __getitem__(self, sl):
        if not isinstance(sl, slice):
            raise TypeError('a FieldTable is sliced, not indexed')
        t = FieldTable(self.rec[sl], self.poly_offsets, self.poly_x, self.poly_y)
        t._pinned = self._pinned    # (a slice of pinned records is pinned, and keeps the buffer alive)
        if self._dev is not None:   # (a contiguous slice of a table on the device is on the device)
            lo, hi, step = sl.indices(len(self))
            if step == 1:
                sz = _field_dtype().itemsize
                t._dev = self._dev[lo * sz:max(lo, hi) * sz]
        return t

    def pin(self):
        """Moves the records into pinned host memory (once; needs a GPU): fcpp_batch_create / fcpp_plan_points then let the device read
        them where they lie instead of copying them first -- for a table that is planned more than once, or built in place.  -> self"""
        if self._pinned is None:
            torch = _torch()
            dt = _field_dtype()
            n = len(self)
            buf = torch.empty(max(n, 1) * dt.itemsize, dtype=torch.uint8, pin_memory=True)
            rec = buf.numpy().view(dt)[:n]
            rec[...] = self.rec
            self.rec, self._pinned, self._cargs = rec, buf, None
        return self

    def to_device(self, device=None):
        """Copies the records into DEVICE memory (once; needs a GPU): fcpp_batch_plan / fcpp_batch_create / fcpp_plan_points then read them
        where they lie -- nothing crosses PCIe in front of the plan call's first kernel (the headline's 512 KB of records were ~10 us of
        it), as for a table whose fields are made on the GPU.  `rec` stays the host's copy (slicing, sharding): records written in place
        afterwards are NOT seen by the library until to_device() is called again on a table with a new `rec`.  The host paths of the library
        (a handful of fields, AVOID mode, FCPP_SETUP=host) copy the records back first.  -> self"""
        if self._dev is None:
            torch = _torch()
            rec = np.ascontiguousarray(self.rec)
            dev = torch.device('cuda', torch.cuda.current_device() if device is None else device)
            self._dev = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(dev)
            self._cargs = None
        return self

    @staticmethod
    def _points(rec, name, pts):
        if pts is None:
            return
        pts = np.asarray(pts, dtype=np.float64).reshape(len(rec), 2)
        has = ~np.isnan(pts).any(axis=1)
        rec['has_' + name] = has
        rec[name + '_x'] = np.where(has, pts[:, 0], 0.0)
        rec[name + '_y'] = np.where(has, pts[:, 1], 0.0)

    @classmethod
    def from_vertices(cls, V, start_points=None, end_points=None):
        V = np.asarray(V, dtype=np.float64)
        if V.ndim != 3 or V.shape[1:] != (4, 2):
            raise ValueError('only quadrilateral fields are supported (4 vertices)')
        rec = np.zeros(V.shape[0], dtype=_field_dtype())
        rec['vx'], rec['vy'] = V[:, :, 0], V[:, :, 1]
        rec['from_vertices'] = 1
        cls._points(rec, 'start', start_points)
        cls._points(rec, 'end', end_points)
        return cls(rec)

    @classmethod
    def from_rectangles(cls, LH, start_points=None, end_points=None):
        LH = np.asarray(LH, dtype=np.float64).reshape(-1, 2)
        rec = np.zeros(LH.shape[0], dtype=_field_dtype())
        rec['vx'][:, 1] = rec['vx'][:, 2] = LH[:, 0]          # (0,0), (L,0), (L,H), (0,H)  (MLP:127-132)
        rec['vy'][:, 2] = rec['vy'][:, 3] = LH[:, 1]
        cls._points(rec, 'start', start_points)
        cls._points(rec, 'end', end_points)
        return cls(rec)

    @classmethod
    def from_specs(cls, specs):
        """Raises ValueError like MLP:135 when a spec names no field."""
        n = len(specs)
        rec = np.zeros(n, dtype=_field_dtype())
        V = np.zeros((n, 4, 2), dtype=np.float64)
        offs, px, py = [0], [], []
        nan2 = (float('nan'), float('nan'))
        starts, ends = [], []
        for i, s in enumerate(specs):
            if s.field_vertices is not None:
                vs = list(s.field_vertices)
                if len(vs) != 4:
                    raise ValueError('only quadrilateral fields are supported (4 vertices)')
                V[i] = vs
                rec['from_vertices'][i] = 1
            elif s.field_length is not None and s.field_width is not None:
                V[i] = ((0.0, 0.0), (s.field_length, 0.0), (s.field_length, s.field_width), (0.0, s.field_width))
            else:
                raise ValueError('必须提供 field_vertices 或 (field_length, field_width)')
            starts.append(nan2 if s.start_point is None else (float(s.start_point[0]), float(s.start_point[1])))
            ends.append(nan2 if s.end_point is None else (float(s.end_point[0]), float(s.end_point[1])))
            obs = s.obstacles or []
            rec['obstacle_first'][i] = len(offs) - 1
            rec['n_obstacles'][i] = len(obs)
            for poly in obs:
                for (x, y) in poly:
                    px.append(float(x))
                    py.append(float(y))
                offs.append(len(px))
        rec['vx'], rec['vy'] = V[:, :, 0], V[:, :, 1]
        cls._points(rec, 'start', np.asarray(starts, dtype=np.float64).reshape(n, 2))
        cls._points(rec, 'end', np.asarray(ends, dtype=np.float64).reshape(n, 2))
        return cls(rec, offs, px, py)

    def c_args(self):
        """-> (fcpp_field pointer, fcpp_polys, objects to keep alive during the call)"""
        if self._cargs is not None:
            return self._cargs
        # (the pointers are kept only when they point INTO self.rec: in-place writes to the records then stay what the library reads.  A
        # non-contiguous view -- table[::2] -- is copied here, at every call, so that writes made since the last one are seen)
        contiguous = self.rec.flags.c_contiguous
        rec = self.rec if contiguous else np.ascontiguousarray(self.rec)
        polys = L.Polys(len(self.poly_offsets) - 1, self.poly_offsets.ctypes.data_as(L.c_i64_p), self.poly_x.ctypes.data_as(L.c_double_p),
                        self.poly_y.ctypes.data_as(L.c_double_p))
        if self._dev is not None:
            cargs = (C.cast(C.c_void_p(self._dev.data_ptr()), C.POINTER(L.Field)), polys, [self._dev, self.poly_offsets, self.poly_x, self.poly_y])
            self._cargs = cargs
            return cargs
        cargs = (C.cast(C.c_void_p(rec.ctypes.data), C.POINTER(L.Field)), polys, [rec, self.poly_offsets, self.poly_x, self.poly_y])
        if contiguous:
            self._cargs = cargs
        return cargs


def as_table(specs):
    return specs if isinstance(specs, FieldTable) else FieldTable.from_specs(specs)


def pack_fields(specs):
    """-> (Field pointer, Polys, keep-alive list).  Raises ValueError like MLP:135 when no field is given."""
    return as_table(specs).c_args()


class InfoTable:
    """fcpp_field_info of n fields: `infos[i]` is the ctypes record (attribute access as before), `infos.array` a numpy record view of
    all of them (`infos.array['n_main']`), `infos.counts()` the points per field -- no Python loop over 65 536 records."""

    def __init__(self, n):
        self.n = int(n)
        self._c = (L.FieldInfo * max(self.n, 1))()
        self.array = np.frombuffer(self._c, dtype=np.dtype(L.FieldInfo))[:self.n]

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._c[k] for k in range(*i.indices(self.n))]
        if i < 0:
            i += self.n
        if not 0 <= i < self.n:
            raise IndexError(i)
        return self._c[i]

    def __iter__(self):
        return (self._c[k] for k in range(self.n))

    def __eq__(self, other):            # (an empty table equals an empty list, as the list this used to be)
        try:
            return len(other) == self.n and all(a is b or bytes(a) == bytes(b) for a, b in zip(self, other))
        except TypeError:
            return NotImplemented

    def counts(self):
        return (self.array['n_main'] + self.array['n_head']).astype(np.int64)


def plan_count(specs, vehicle, options):
    """Host-only sizing/decisions (fcpp_plan_count); needs no GPU.  -> InfoTable"""
    lib = L.load()
    arr, polys, _keep = pack_fields(specs)
    info = InfoTable(len(specs))
    L.check(lib.fcpp_plan_count(C.byref(vehicle), C.byref(options), len(specs), arr, C.byref(polys), info._c))
    return info


def plan_points(specs, vehicle, options, device=None):
    """Points per field (n_main + n_head; 0 for a field that raises) as a numpy int64 array: the sizing a sharded job cuts its blocks on
    (fcpp_plan_points).  Computed on the GPU where the device-side setup takes the batch, else on the host."""
    ctx = get_context(device)
    arr, polys, _keep = pack_fields(specs)
    out = np.zeros(len(specs), dtype=np.int64)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_plan_points(ctx.handle, C.byref(vehicle), C.byref(options), len(specs), arr, C.byref(polys), out.ctypes.data_as(L.c_i64_p)))
    return out


class _ArenaArrays:
    """Five output arrays from the context's arena (fcpp_outputs_alloc), handed to torch as views of the library's memory through the CUDA
    array interface; the allocation goes back to the arena when the last view is gone."""

    class _View:
        def __init__(self, owner, ptr, n, typestr):
            self._owner = owner
            self.__cuda_array_interface__ = {'shape': (n,), 'typestr': typestr, 'data': (ptr, False), 'version': 2, 'strides': None}

    def __init__(self, ctx, n_points, ptrs=None):
        self.ctx = ctx
        if ptrs is None:
            ptrs = [C.c_void_p() for _ in range(5)]
            L.check(ctx.lib.fcpp_outputs_alloc(ctx.handle, int(n_points), 0, *[C.byref(q) for q in ptrs]))
            ptrs = [q.value for q in ptrs]
        self.ptrs = list(ptrs)          # (given: arrays the library has already allocated -- fcpp_batch_plan -- which this object now owns)

    def tensors(self, n_points):
        torch = _torch()
        dev = torch.device('cuda', self.ctx.device)
        out = []
        for k, p in enumerate(self.ptrs):
            v = self._View(self, p, int(n_points), '<f8' if k < 4 else '<i4')
            t = torch.as_tensor(v, device=dev)
            t._fcpp_owner = v               # (the view object -- and through it this allocation -- lives as long as the tensor object)
            out.append(t)
        return out

    def __del__(self):
        try:
            if getattr(self, 'ptrs', None) and self.ctx.handle:
                self.ctx.lib.fcpp_outputs_free(self.ctx.handle, C.c_void_p(self.ptrs[0]))
                self.ptrs = None
        except Exception:
            pass


class _StatsView:
    """The statistics records a batch keeps in its own device allocation (fcpp_batch_own_stats), handed to torch through the CUDA array
    interface; the batch's close() waits for the last tensor made from this view."""

    def __init__(self, batch, ptr, n_words):
        self._batch = batch
        self.__cuda_array_interface__ = {'shape': (n_words,), 'typestr': '<i8', 'data': (ptr, False), 'version': 2, 'strides': None}

    def __del__(self):
        try:
            b = self._batch
            b._stats_views = 0
            if getattr(b, '_close_pending', False):
                b.close()
        except Exception:
            pass


class BatchResult:
    """Device-resident result of one batch: SoA tensors + per-field stats."""

    def __init__(self, batch, x, y, kappa, v, flagseg, stats_raw):
        self.batch, self.x, self.y, self.kappa, self.v, self.flagseg = batch, x, y, kappa, v, flagseg
        self.stats_raw = stats_raw   # (n_fields, 13) int64 view of fcpp_field_stats

    def stats(self):
        """-> dict of numpy arrays, one entry per field."""
        raw = self.stats_raw.cpu().numpy()
        names = [n for n, _ in L.FieldStats._fields_]
        out = {}
        for k, n in enumerate(names):
            col = raw[:, k]
            out[n] = col.view(np.float64).copy() if k < L.STATS_DOUBLES else col.copy()
        return out

    def field_slice(self, i):
        info = self.batch.info[i]
        return slice(info.point_offset, info.point_offset + info.n_main + info.n_head)

    def path_offsets(self):
        """CSR offsets (numpy int64, 2 * n_fields + 1) of the batch's paths as the trajectory entries see them: two per field, main work
        then headland; a field that raised is two empty paths."""
        a = self.batch.info.array
        off = np.zeros(2 * len(a) + 1, dtype=np.int64)
        off[1::2], off[2::2] = a['n_main'], a['n_head']
        return np.cumsum(off)

    def trajectory(self):
        """-> (s, t, heading, totals): arc length [m], time stamp [s] and vehicle heading [rad, (-pi, pi]] of every point of the batch
        arrays, each counted from the start of its own path (path_offsets(): main work and headland are timed separately, MLP:423-431), and
        totals of shape (n_fields, 4) = main length, main time, headland length, headland time (fcpp_batch_trajectory)."""
        torch = _torch()
        b = self.batch
        s, t, h = torch.empty_like(self.x), torch.empty_like(self.x), torch.empty_like(self.x)
        totals = torch.zeros((b.n_fields, 4), dtype=torch.float64, device=self.x.device)
        b.ctx.bind_stream()
        L.check(b.lib.fcpp_batch_trajectory(b.handle, _ptr(self.x), _ptr(self.y), _ptr(self.v), _ptr(self.flagseg), _ptr(s), _ptr(t), _ptr(h),
                                            _ptr(totals)))
        return s, t, h, totals

    def sample(self, dt, include_end=True):
        """The batch's trajectories at a fixed time step dt [s] -> dict as trajectory_sample(); sample range out_offsets[2 f] ..
        out_offsets[2 f + 1] is field f's main work, the next range its headland."""
        s, t, h, totals = self.trajectory()
        return _sample(self.batch.ctx, self.x, self.y, self.v, self.flagseg, self.path_offsets(), None, (s, t, h, totals.view(-1, 2)), dt, include_end)


    def drivable_connectors(self, radius=None, spacing=0.5, start_headings=None, end_headings=None, reversing=False):
        """Connectors a vehicle with a turning radius can drive, in place of the reference's straight lines (MLP:1313-1355): per field up to
        three Dubins paths (fcpp_dubins_solve / _counts / _sample) --
          0 approach:  parking pose -> the first point of the headland path (`approach_to`) with that point's heading; fields with a kept start point
          1 link:      last point of the main work with its heading -> first point of the headland with its heading; fields with both paths
          2 departure: last point of the headland path (`departure_from`) with its heading -> parking pose; fields with a kept end point
        radius: default the vehicle's min_turn_radius.  start_headings / end_headings: the parking headings [rad], a scalar or one per field;
        default the direction of the reference's straight connector.  The poses on the coverage path are gathered on the device from the batch
        arrays and from trajectory()'s headings.  Fields that raised have no connectors.
        -> dict: 'x', 'y', 'heading', 'kappa' (device, one entry per sample), 'offsets' (device) / 'offsets_host' (numpy): CSR over the
        connectors, 'field' and 'kind' (numpy, per connector, sorted by field then kind), 'length', 'word', 'from_poses', 'to_poses' (device).
        reversing: the same three connectors as Reeds-Shepp paths (fcpp_rs_solve / _counts / _sample) for a vehicle that also backs up: never
        longer, and a three-point turn where the swaths lie closer than two radii.  The dict gains 'gear' (int8 per sample: +1 forward, -1
        reverse; every cusp is two samples with one pose and opposite gears), 'seg' has five signed lengths and 'word' indexes the 48-word
        table of include/fcpp.h."""
        torch = _torch()
        b = self.batch
        a = b.info.array
        dev = self.x.device
        R = float(b.vehicle.min_turn_radius if radius is None else radius)
        ok = a['status'] == 0
        first_head = a['point_offset'] + a['n_main']
        has = (ok & (a['start_kept'] != 0) & (a['n_head'] > 0), ok & (a['n_main'] > 0) & (a['n_head'] > 0), ok & (a['end_kept'] != 0) & (a['n_head'] > 0))
        field = np.concatenate([np.flatnonzero(h) for h in has]).astype(np.int64)
        kind = np.concatenate([np.full(int(h.sum()), k, dtype=np.int32) for k, h in enumerate(has)])
        order = np.lexsort((kind, field))
        field, kind = field[order], kind[order]
        m = len(field)
        # indices into the batch arrays of the poses that lie on the coverage path (0 where the pose is the parking pose), and the parking points
        fi = np.where(kind == 1, first_head[field] - 1, np.where(kind == 2, first_head[field] + a['n_head'][field] - 1, 0))
        ti = np.where(kind == 2, 0, first_head[field])
        park = np.where((kind == 0)[:, None], a['approach_from'][field], a['departure_to'][field]).reshape(m, 2)
        heads = np.full(m, np.nan)
        for k, given in ((0, start_headings), (2, end_headings)):
            if given is not None:
                g = np.broadcast_to(np.asarray(given, dtype=np.float64), (b.n_fields,))
                heads[kind == k] = g[field[kind == k]]
        h = self.trajectory()[2]
        fi_d, ti_d = torch.as_tensor(fi, device=dev), torch.as_tensor(ti, device=dev)
        kind_d = torch.as_tensor(kind, device=dev)
        park_d, heads_d = torch.as_tensor(park, device=dev), torch.as_tensor(heads, device=dev)
        if self.x.numel() == 0:
            fi_d, ti_d = fi_d[:0], ti_d[:0]
        frm = torch.stack((self.x[fi_d], self.y[fi_d], h[fi_d]), dim=1)
        to = torch.stack((self.x[ti_d], self.y[ti_d], h[ti_d]), dim=1)
        is_ap, is_dp = (kind_d == 0)[:, None], (kind_d == 2)[:, None]
        # the parking pose: its heading as given, else along the straight connector of the reference (parking -> path / path -> parking)
        ap_dir = torch.atan2(to[:, 1] - park_d[:, 1], to[:, 0] - park_d[:, 0])
        dp_dir = torch.atan2(park_d[:, 1] - frm[:, 1], park_d[:, 0] - frm[:, 0])
        given = ~torch.isnan(heads_d)
        ap_pose = torch.cat((park_d, torch.where(given, heads_d, ap_dir)[:, None]), dim=1)
        dp_pose = torch.cat((park_d, torch.where(given, heads_d, dp_dir)[:, None]), dim=1)
        frm = torch.where(is_ap, ap_pose, frm)
        to = torch.where(is_dp, dp_pose, to)
        out = _conn_paths(b.ctx, frm, to, R, spacing, reversing)
        out.update(field=field, kind=kind, from_poses=frm, to_poses=to, radius=R)
        return out


class Batch:
    """n independent fields planned together on one GPU (fcpp_batch_*)."""

    def __init__(self, specs, vehicle, options=None, device=None):
        self.ctx = get_context(device)
        self.lib = self.ctx.lib
        self.vehicle = vehicle
        self.options = options or make_options()
        self.n_fields = len(specs)
        import time
        t0 = time.perf_counter()
        arr, polys, _keep = pack_fields(specs)
        self.pack_ms = (time.perf_counter() - t0) * 1e3          # (0 for a FieldTable the caller already holds)
        self.ctx.bind_stream()
        h = C.c_void_p()
        L.check(self.lib.fcpp_batch_create(self.ctx.handle, C.byref(self.vehicle), C.byref(self.options),
                                           self.n_fields, arr, C.byref(polys), C.byref(h)))
        self.handle = h
        self._info = None
        self._token = object()      # marks the buffers alloc() makes for this batch
        tot = C.c_int64()
        L.check(self.lib.fcpp_batch_info(self.handle, None, C.byref(tot)))
        self.total_points = tot.value
        self._last_mode = 1

    @classmethod
    def plan(cls, specs, vehicle, options=None, device=None):
        """The reference's plan call for a whole batch in ONE library call (fcpp_batch_plan: plan_complete_coverage, MLP:387-465, sets a new
        field up and generates its path): batch creation, its output arrays (from the context's arena when it has one) and one step, with
        no Python between them.  -> (Batch, BatchResult), asynchronous like run(); the buffers of the result serve further run() calls."""
        torch = _torch()
        self = cls.__new__(cls)
        self.ctx = get_context(device)
        self.lib = self.ctx.lib
        self.vehicle = vehicle
        self.options = options or make_options()
        self.n_fields = len(specs)
        arr, polys, _keep = pack_fields(specs)
        self.pack_ms = 0.0
        self._info = None
        self._token = object()
        self._last_mode = 1
        self.ctx.bind_stream()
        h = C.c_void_p()
        ptrs = [C.c_void_p() for _ in range(5)]
        tot = C.c_int64()
        # (no statistics records of ours: the batch's own, inside its device allocation -- nothing is allocated in front of the call, and
        # whatever Python can do behind it -- the device object, the tensors over the arrays -- is done while the device works)
        L.check(self.lib.fcpp_batch_plan(self.ctx.handle, C.byref(self.vehicle), C.byref(self.options), self.n_fields, arr, C.byref(polys),
                                         None, C.byref(h), *[C.byref(q) for q in ptrs], C.byref(tot)))
        dev = torch.device('cuda', self.ctx.device)
        self.handle = h
        self.total_points = n = tot.value
        sp = C.c_void_p()
        L.check(self.lib.fcpp_batch_own_stats(h, C.byref(sp)))
        if self.n_fields > 0 and sp.value:
            # (a view of the batch's own memory: while a tensor made from it is alive, close() only marks the batch -- the tables are
            # released when the last such tensor is gone)
            sv = _StatsView(self, sp.value, self.n_fields * L.STATS_WORDS)
            stats = torch.as_tensor(sv, device=dev).view(self.n_fields, L.STATS_WORDS)
            stats._fcpp_owner = sv
            self._stats_views = 1
        else:
            stats = torch.empty((self.n_fields, L.STATS_WORDS), dtype=torch.int64, device=dev)
        owner = _ArenaArrays(self.ctx, n, [q.value or 0 for q in ptrs])
        if n > 0:
            x, y, kappa, v, fs = owner.tensors(n)
        else:
            x, y, kappa, v = (torch.empty(0, dtype=torch.float64, device=dev) for _ in range(4))
            fs = torch.empty(0, dtype=torch.int32, device=dev)
            x._fcpp_owner = owner
        lane, pitch = self.ctx.arena()
        self.layout = {'layout': 'arena' if (n > 0 and pitch and owner.ptrs[1] - owner.ptrs[0] == pitch) else 'plain', 'one_call': True}
        bufs = self._trusted((x, y, kappa, v, fs, stats))
        return self, BatchResult(self, *bufs)

    @property
    def info(self):
        """fcpp_field_info of every field (InfoTable).  A batch set up on the device keeps the records there until they are asked for:
        the first access copies them back (and waits for the batch's setup)."""
        if self._info is None:
            t = InfoTable(self.n_fields)
            L.check(self.lib.fcpp_batch_info(self.handle, t._c, None))
            self._info = t
        return self._info

    def setup_times(self):
        """Where the time of this batch's creation went, in ms: {'pack', 'host_plan', 'templates', 'tiler', 'image', 'h2d', 'create'
        (the fcpp_batch_create call), 'threads', 'image_bytes'}.  The plan call the reference times (plan_complete_coverage,
        MLP:387-465) = this + one run()."""
        t = L.SetupTimes()
        L.check(self.lib.fcpp_batch_setup_times(self.handle, C.byref(t)))
        return {'pack': self.pack_ms, 'host_plan': t.host_plan_ms, 'templates': t.templates_ms, 'tiler': t.tiler_ms, 'image': t.image_ms,
                'h2d': t.h2d_ms, 'create': t.total_ms, 'threads': int(t.threads), 'image_bytes': int(t.image_bytes),
                'device_setup': int(t.device_setup)}

    def setup_path(self):
        """'device' if this batch was set up on the GPU (fcpp_devplan), else 'host'"""
        t = L.SetupTimes()
        L.check(self.lib.fcpp_batch_setup_times(self.handle, C.byref(t)))
        return 'device' if t.device_setup else 'host'

    def debug_table(self, table):
        """One of the batch's device tables as bytes (fcpp_batch_debug_table; tests)."""
        nb = C.c_int64()
        L.check(self.lib.fcpp_batch_debug_table(self.handle, int(table), None, 0, C.byref(nb)))
        buf = np.zeros(max(nb.value, 1), dtype=np.uint8)
        L.check(self.lib.fcpp_batch_debug_table(self.handle, int(table), C.c_void_p(buf.ctypes.data), nb.value, C.byref(nb)))
        return buf[:nb.value]

    SPREAD_MIN_BYTES = 512 << 20        # batches with less output than this live in the caches: placement does not matter

    def alloc(self, layout='auto', best_of=1, include=()):
        """Output buffers (x, y, kappa, v, flagseg, stats) for run().

        layout: where the five arrays lie in device memory.  The hot kernels write them side by side, and on MI355X five write streams
        that lie within a few GiB of each other reach 4.6 TB/s where the same streams 12-24 GiB or more apart reach 6.3-6.6 TB/s
        (HISTORY.md; tools/placement_pitch.py: the speed class follows the pitch between the arrays, nothing else).
          'spread': ONE allocation, the arrays L.OUTPUT_PITCH (24 GiB) + their own size apart (less if the device has less room); the gaps
                    belong to the allocation -- a caller that needs them sub-allocates its own slab with the same rule.
          'plain' : five separate tensors, wherever the allocator puts them (usually back to back: the slow class).
          'arena' : from the context's output arena (Context.reserve_outputs(): one allocation made once, five lanes a pitch apart, shared
                    by all live batches) -- the spread placement without an allocation per batch.
          'auto'  : 'arena' when the context has one and the arrays are large enough to matter (>= 512 MiB of output), else 'plain'.
                    (Never 'spread': an allocation of ~100 GiB is not something a default should make.)
        self.layout tells which one was used and the pitch.

        best_of > 1 (opt-in, round 2's remedy): `best_of` further candidate sets are allocated ('plain'), the batch's own step is timed on
        each (and on the sets in `include`), the fastest is kept (`self.placement`).  Setup work; never inside a timed region; not what
        bench.py reports as its primary figures."""
        if best_of > 1 and self.total_points > 0:
            torch = _torch()
            import time
            dev = torch.device('cuda', self.ctx.device)
            sets, ms = list(include), []
            for _ in range(int(best_of)):
                try:
                    sets.append(self._alloc_once())
                except RuntimeError:          # out of device memory: choose among what we have
                    break
            if not sets:
                raise RuntimeError(f'out of device memory: no candidate set of output arrays ({36 * self.total_points / 2**30:.1f} GiB each) could be allocated')
            for s in sets:
                self.run(s)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(3):
                    self.run(s)
                torch.cuda.synchronize(dev)
                ms.append((time.perf_counter() - t0) / 3 * 1e3)
            k = min(range(len(sets)), key=lambda i: ms[i])
            self.placement = {'probe': 'step', 'step_ms': [round(v, 4) for v in ms], 'chosen': k}
            keep = sets[k]
            del sets
            torch.cuda.empty_cache()
            return keep
        if layout not in ('auto', 'plain', 'spread', 'arena'):
            raise ValueError("layout: 'auto', 'plain', 'spread' or 'arena'")
        n = self.total_points
        lane, pitch = self.ctx.arena()
        if layout == 'arena' or (layout == 'auto' and lane >= 8 * n and 36 * n >= self.SPREAD_MIN_BYTES):
            # the context's arena (Context.reserve_outputs): array k in lane k, a pitch apart, shared with every other live batch
            if lane < 8 * n:
                raise RuntimeError('the context has no output arena of that size: Context.reserve_outputs()')
            torch = _torch()
            arr = _ArenaArrays(self.ctx, n)
            if arr.ptrs[1] - arr.ptrs[0] != pitch:        # (the arena was full: the library fell back to an allocation of its own)
                self.layout = {'layout': 'plain', 'note': 'the output arena is full'}
            else:
                self.layout = {'layout': 'arena', 'pitch_GiB': round(pitch / 2**30, 3), 'lane_GiB': round(lane / 2**30, 3)}
            x, y, kappa, v, fs = arr.tensors(n)
            stats = torch.empty((self.n_fields, L.STATS_WORDS), dtype=torch.int64, device=torch.device('cuda', self.ctx.device))
            return self._trusted((x, y, kappa, v, fs, stats))
        if layout in ('plain', 'auto'):
            # ('auto' never takes device memory the arrays do not need: the spread placement is the arena's, or an explicit layout='spread')
            self.layout = {'layout': 'plain'}
            return self._trusted(self._alloc_once())
        return self._trusted(self._alloc_spread(strict=True))

    def _trusted(self, buffers):
        """buffers alloc() has just made carry this batch's token: run() does not check them again (no reference to them is kept here:
        they go back to the allocator / the arena when the caller drops them)"""
        tok = self._token
        for t in buffers:
            t._fcpp_ok = tok
        return buffers

    def _alloc_spread(self, strict=False):
        torch = _torch()
        dev = torch.device('cuda', self.ctx.device)
        n = self.total_points
        S = (8 * n + 4095) // 4096 * 4096
        free, _total = torch.cuda.mem_get_info(dev)
        free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)       # (what the caching allocator could hand back)
        reserve = 8 << 30
        P = max(L.OUTPUT_PITCH, S + (1 << 30))
        if free < 4 * P + S + reserve:
            P = (free - reserve - S) // 4 if free > 5 * S + reserve else 0
        P = P // 4096 * 4096
        if P < S + (1 << 30) and not strict:       # no room to spread: the plain layout
            self.layout = {'layout': 'plain', 'note': 'no room for the spread layout'}
            return self._alloc_once()
        P = max(P, S)
        try:
            slab = torch.empty(4 * P + S, dtype=torch.uint8, device=dev)
        except RuntimeError:
            if strict:
                raise
            self.layout = {'layout': 'plain', 'note': 'the spread allocation failed'}
            return self._alloc_once()
        x, y, kappa, v = (slab[k * P: k * P + 8 * n].view(torch.float64) for k in range(4))
        fs = slab[4 * P: 4 * P + 4 * n].view(torch.int32)
        stats = torch.empty((self.n_fields, L.STATS_WORDS), dtype=torch.int64, device=dev)
        self.layout = {'layout': 'spread', 'pitch_GiB': round(P / 2**30, 3), 'allocation_GiB': round((4 * P + S) / 2**30, 3)}
        return x, y, kappa, v, fs, stats

    def _alloc_once(self):
        torch = _torch()
        dev = torch.device('cuda', self.ctx.device)
        n = self.total_points
        # (the four float64 arrays: rows of one allocation, each on a 512-byte boundary -- one call to the allocator instead of four)
        npad = (n + 63) // 64 * 64
        x, y, kappa, v = torch.empty((4, npad), dtype=torch.float64, device=dev)[:, :n].unbind(0)
        fs = torch.empty(n, dtype=torch.int32, device=dev)
        # (not cleared: fcpp_batch_run writes every field's row, zeros for a field that raised -- a fill kernel here would sit in the
        # stream in front of the step)
        stats = torch.empty((self.n_fields, L.STATS_WORDS), dtype=torch.int64, device=dev)
        return x, y, kappa, v, fs, stats

    def _check_buffers(self, buffers):
        """The library writes total_points elements into each array without looking at it again: sizes, types, device and layout
        are checked here (a short buffer would be an out-of-bounds device write)."""
        torch = _torch()
        x, y, kappa, v, fs, stats = buffers
        want = [('x', x, torch.float64, self.total_points), ('y', y, torch.float64, self.total_points),
                ('kappa', kappa, torch.float64, self.total_points), ('v', v, torch.float64, self.total_points),
                ('flagseg', fs, None, self.total_points), ('stats', stats, torch.int64, self.n_fields * L.STATS_WORDS)]
        for name, t, dtype, numel in want:
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device.index != self.ctx.device:
                raise ValueError(f'{name}: expected a tensor on cuda:{self.ctx.device}')
            if dtype is None:
                if t.dtype not in (torch.int32, torch.uint32):
                    raise ValueError(f'{name}: expected int32 / uint32, got {t.dtype}')
            elif t.dtype != dtype:
                raise ValueError(f'{name}: expected {dtype}, got {t.dtype}')
            if t.numel() < numel or not t.is_contiguous():
                raise ValueError(f'{name}: needs {numel} contiguous elements, got {t.numel()}')

    def run(self, buffers=None, mode=1):
        """Enqueue the hot path on torch's current stream; returns a BatchResult (asynchronous)."""
        if buffers is None:
            buffers = self.alloc()
        tok = self._token
        for t in buffers:
            if getattr(t, '_fcpp_ok', None) is not tok:
                self._check_buffers(buffers)
                break
        x, y, kappa, v, fs, stats = buffers
        self._last_mode = 1 if int(mode) >= 1 else 0
        self.ctx.bind_stream()
        L.check(self.lib.fcpp_batch_run(self.handle, _ptr(x), _ptr(y), _ptr(kappa), _ptr(v), _ptr(fs), _ptr(stats),
                                        int(mode)))
        return BatchResult(self, x, y, kappa, v, fs, stats)

    def connectors(self):
        """-> (approach, departure) tensors of shape (n_fields, 50, 2); rows of fields without a kept
        start/end point are NaN."""
        torch = _torch()
        dev = torch.device('cuda', self.ctx.device)
        ap = torch.full((self.n_fields, 50, 2), float('nan'), dtype=torch.float64, device=dev)
        dp = torch.full((self.n_fields, 50, 2), float('nan'), dtype=torch.float64, device=dev)
        self.ctx.bind_stream()
        L.check(self.lib.fcpp_batch_connectors(self.handle, _ptr(ap), _ptr(dp)))
        return ap, dp

    def set_profiling(self, on=True, every=1):
        """Per-kernel HIP-event timing of every `every`-th run() from now on (on=False: off)."""
        L.check(self.lib.fcpp_batch_set_profiling(self.handle, int(every) if on else 0))

    def stage_times(self):
        """-> ({kernel name: mean ms per run}, runs) from the HIP events recorded since the last call."""
        ms = (C.c_double * 16)()
        ns, nr = C.c_int(), C.c_int()
        L.check(self.lib.fcpp_batch_stage_times(self.handle, 16, ms, C.byref(ns), C.byref(nr)))
        runs = max(nr.value, 1)
        return {self.lib.fcpp_batch_stage_name(self._last_mode, k).decode(): ms[k] / runs for k in range(ns.value)}, nr.value

    def stage_points(self):
        """-> {kernel name: points one launch of it processes} for the pipeline of the last run()."""
        out = {}
        k = 0
        while True:
            name = self.lib.fcpp_batch_stage_name(self._last_mode, k).decode()
            if not name:
                break
            n = C.c_int64()
            L.check(self.lib.fcpp_batch_stage_points(self.handle, self._last_mode, k, C.byref(n)))
            out[name] = n.value
            k += 1
        return out

    def reduce_classes(self):
        """-> [paths whose statistics 8 lanes / a wavefront / a workgroup / 64 workgroups reduce] (fused pipeline)"""
        out = (C.c_int64 * 4)()
        L.check(self.lib.fcpp_batch_reduce_classes(self.handle, out))
        return list(out)

    def point_split(self):
        """-> (points handled by k_plan_quiet, points handled by k_plan_fused) in the fused pipeline."""
        q, g = C.c_int64(), C.c_int64()
        L.check(self.lib.fcpp_batch_point_split(self.handle, C.byref(q), C.byref(g)))
        return q.value, g.value

    def close(self):
        if getattr(self, 'handle', None):
            if getattr(self, '_stats_views', 0):        # (a result of plan() still reads the batch's own statistics records)
                self._close_pending = True
                return
            self.lib.fcpp_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- standalone operators on device tensors -------------------------------------------------------
def _dev_f64(a, device):
    torch = _torch()
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=device)


def _offsets(offsets, n, device):
    """-> (device tensor, host numpy copy or None): CSR offsets of the paths.  Host-side offsets (lists, numpy) are handed to the
    library as they are, so it need not read the device copy back."""
    torch = _torch()
    if offsets is None:
        offsets = [0, n]
    if isinstance(offsets, torch.Tensor):
        if offsets.is_cuda:
            return offsets.to(device=device, dtype=torch.int64).contiguous(), None
        offsets = offsets.numpy()
    host = np.ascontiguousarray(offsets, dtype=np.int64)
    return torch.as_tensor(host, device=device), host


def _host_ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


# ---- the CSR toolkit of the polygon chain's bindings ("the binding layer") -------------------------------------------------
def _owners(off, total, dtype=None):
    """the row of every element of a CSR table with the (n + 1) offsets `off`: (total) int64, or `dtype`, on off's device"""
    torch = _torch()
    rows = torch.arange(int(off.numel()) - 1, dtype=dtype or torch.int64, device=off.device)
    return torch.repeat_interleave(rows, off[1:] - off[:-1], output_size=total)


def _one_per(t, n, name, each):
    """a tensor of one value, or of one value per `each`, as n contiguous values; ValueError in the words of `name`"""
    t = t.reshape(-1)
    if t.numel() == 1 and n != 1:
        t = t.expand(n)
    if t.numel() != n:
        raise ValueError('%s must be a scalar or hold one %s' % (name, each))
    return t.contiguous()


def _join_csr(offsets, hosts, columns, dtypes, dev):
    """Several CSR tables laid end to end.  offsets[k]: table k's (n_k + 1) offsets, a tensor; hosts[k]: their numpy copy or None;
    columns[k]: its element columns, one per entry of `dtypes` -> (first, starts, offsets, offsets_host, columns): where table k's rows
    and elements start in the join (numpy, one value more than tables), the shifted offsets on `dev`, their host copy when every table
    brought one (else None), the concatenated columns."""
    torch = _torch()
    first = np.concatenate([[0], np.cumsum([int(o.numel()) - 1 for o in offsets])]).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum([int(c[0].numel()) for c in columns])]).astype(np.int64)
    total = int(starts[-1])
    cols = [(torch.cat([c[j].to(dev) for c in columns]) if columns else torch.empty(0, dtype=dt, device=dev)).contiguous()
            for j, dt in enumerate(dtypes)]
    off = torch.cat([o[:-1].to(dev) + int(starts[k]) for k, o in enumerate(offsets)] + [torch.full((1,), total, dtype=torch.int64, device=dev)]).contiguous()
    off_h = None
    if all(h is not None for h in hosts):
        off_h = np.ascontiguousarray(np.concatenate([np.asarray(h[:-1], dtype=np.int64) + starts[k] for k, h in enumerate(hosts)] + [[total]]),
                                     dtype=np.int64)
    return first, starts, off, off_h, cols


def _group_by(owner, n, error=None):
    """rows by owner -> (order, group_offsets): the stable order that sorts `owner` (an owner's rows stay as given) and the (n + 1) offsets
    of owners 0 .. n - 1 within it.  error: the ValueError's text for an owner outside 0 .. n - 1; None does not look (such rows then
    belong to no group)."""
    torch = _torch()
    if error is not None and int(owner.numel()) and bool(((owner < 0) | (owner >= n)).any()):
        raise ValueError(error)
    order = torch.argsort(owner, stable=True)
    return order, torch.searchsorted(owner[order], torch.arange(n + 1, dtype=torch.int64, device=owner.device)).to(torch.int64).contiguous()


def _counts_fill(n, dev, counts, fill, columns):
    """The two-call shape of every operator that sizes its own output: (n + 1) offsets and their host copy, the counts entry --
    counts(offsets, offsets_host), pointers -- writes both; the total is read from the HOST copy; one column of `total` elements per dtype of
    `columns`; fill(offsets, offsets_host, total, *columns) -> (offsets, offsets_host, *columns).  No stream is bound here."""
    torch = _torch()
    off, off_h = torch.empty(n + 1, dtype=torch.int64, device=dev), np.zeros(n + 1, dtype=np.int64)
    L.check(counts(_ptr(off), _host_ptr(off_h)))
    total = int(off_h[-1])
    cols = [torch.empty(total, dtype=dt, device=dev) for dt in columns]
    L.check(fill(_ptr(off), _host_ptr(off_h), total, *[_ptr(c) for c in cols]))
    return (off, off_h, *cols)


def _sample_columns(*extra):
    """the dtypes of a path set's six sample columns x, y, heading, kappa, part, gear, and of the caller's behind them"""
    torch = _torch()
    return (torch.float64,) * 4 + (torch.int8,) * 2 + extra


def curvature(x, y, offsets=None, device=None):
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    x, y = _dev_f64(x, dev), _dev_f64(y, dev)
    off, off_h = _offsets(offsets, x.numel(), dev)
    k = torch.empty_like(x)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_curvature(ctx.handle, off.numel() - 1, _ptr(off), x.numel(), _ptr(x), _ptr(y), _ptr(k), _host_ptr(off_h)))
    return k


def speed_plan(x, y, v, vehicle, clamp=True, offsets=None, device=None, want_kappa=False):
    """_apply_curvature_based_speed_limit (clamp=True) or _smooth_speed_profile only (clamp=False)."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    x, y, v = _dev_f64(x, dev), _dev_f64(y, dev), _dev_f64(v, dev)
    off, off_h = _offsets(offsets, x.numel(), dev)
    out = torch.empty_like(v)
    kap = torch.empty_like(v) if want_kappa else None
    nadj = torch.zeros(off.numel() - 1, dtype=torch.int64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_speed_plan(ctx.handle, C.byref(vehicle), int(bool(clamp)), off.numel() - 1, _ptr(off),
                                    x.numel(), _ptr(x), _ptr(y), _ptr(v), _ptr(out), _ptr(kap), _ptr(nadj), _host_ptr(off_h)))
    return (out, nadj, kap) if want_kappa else (out, nadj)


def verify(x, y, v, vehicle, offsets=None, device=None):
    """-> dict of numpy arrays per path (fcpp_verify)."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    x, y, v = _dev_f64(x, dev), _dev_f64(y, dev), _dev_f64(v, dev)
    off, off_h = _offsets(offsets, x.numel(), dev)
    n_paths = off.numel() - 1
    stats = torch.zeros((n_paths, L.STATS_WORDS), dtype=torch.int64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_verify(ctx.handle, C.byref(vehicle), n_paths, _ptr(off), x.numel(), _ptr(x), _ptr(y),
                                _ptr(v), _ptr(stats), _host_ptr(off_h)))
    raw = stats.cpu().numpy()
    out = {}
    for k, (n, _) in enumerate(L.FieldStats._fields_):
        col = raw[:, k]
        out[n] = col.view(np.float64).copy() if k < L.STATS_DOUBLES else col.copy()
    return out


def _dev_flags(a, device):
    """flag / segment words as an int32 device tensor (torch has no uint32 arithmetic; the bits are what matters)"""
    torch = _torch()
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.int32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a).astype(np.uint32, copy=False).view(np.int32), device=device)


def trajectory(x, y, v, flagseg=None, offsets=None, device=None):
    """-> (s, t, heading, totals) device tensors (fcpp_trajectory): per point the arc length [m] and the time stamp [s] counted from its
    path's first point -- the running values of _calculate_path_length / _calculate_work_time, MLP:1290-1311 -- and the vehicle's heading
    [rad, (-pi, pi]]: the chord that leaves the point, carried over zero steps, turned by pi where flagseg says FCPP_KIND_REVERSE;
    totals[p] = (length, time) of path p."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    x, y, v = _dev_f64(x, dev), _dev_f64(y, dev), _dev_f64(v, dev)
    fs = _dev_flags(flagseg, dev)
    off, off_h = _offsets(offsets, x.numel(), dev)
    n_paths = off.numel() - 1
    s, t, h = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    totals = torch.zeros((n_paths, 2), dtype=torch.float64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_trajectory(ctx.handle, n_paths, _ptr(off), x.numel(), _ptr(x), _ptr(y), _ptr(v), _ptr(fs), _ptr(s), _ptr(t), _ptr(h),
                                    _ptr(totals), _host_ptr(off_h)))
    return s, t, h, totals


def _sample(ctx, x, y, v, fs, off_h, off, traj, dt, include_end):
    torch = _torch()
    dev = x.device
    s, t, h, totals = traj
    if off is None:
        off = torch.as_tensor(off_h, device=dev)
    n_paths = off.numel() - 1
    out_off = torch.empty(n_paths + 1, dtype=torch.int64, device=dev)
    out_h = np.zeros(n_paths + 1, dtype=np.int64)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_trajectory_counts(ctx.handle, n_paths, _ptr(totals), float(dt), int(bool(include_end)), _ptr(out_off), _host_ptr(out_h)))
    m = int(out_h[-1])
    out = {k: torch.empty(m, dtype=torch.float64, device=dev) for k in ('x', 'y', 'v', 's', 'heading')}
    out['flagseg'] = torch.empty(m, dtype=torch.int32, device=dev)
    out['src_index'] = torch.empty(m, dtype=torch.int64, device=dev)
    L.check(ctx.lib.fcpp_trajectory_sample(ctx.handle, n_paths, _ptr(off), x.numel(), _ptr(x), _ptr(y), _ptr(v), _ptr(s), _ptr(t), _ptr(h), _ptr(fs),
                                           float(dt), int(bool(include_end)), _ptr(out_off), m, _ptr(out['x']), _ptr(out['y']), _ptr(out['v']),
                                           _ptr(out['s']), _ptr(out['heading']), _ptr(out['flagseg']), _ptr(out['src_index']),
                                           _host_ptr(off_h), _host_ptr(out_h)))
    out['out_offsets'] = out_off
    out['totals'] = totals
    out['out_offsets_host'] = out_h
    out['dt'] = float(dt)
    return out


def trajectory_sample(x, y, v, dt, flagseg=None, offsets=None, include_end=True, device=None, traj=None):
    """The trajectories of the paths at a fixed time step dt [s] (fcpp_trajectory_counts + fcpp_trajectory_sample) -> dict of device
    tensors 'x', 'y', 'v', 's', 'heading', 'flagseg', 'src_index' (one entry per sample; sample k of path p lies at time k * dt and at
    index out_offsets[p] + k), 'out_offsets' (n_paths + 1, device; 'out_offsets_host': numpy), 'totals' (length, time per path) and 'dt'.  x, y, s are interpolated linearly
    within the step the sample falls in, v linearly in time; heading, flag word and src_index are those of the step's first point.  With
    include_end the last sample of every path is its last point.  traj: the (s, t, heading, totals) of trajectory() for the same paths,
    when the caller has them already."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    x, y, v = _dev_f64(x, dev), _dev_f64(y, dev), _dev_f64(v, dev)
    fs = _dev_flags(flagseg, dev)
    off, off_h = _offsets(offsets, x.numel(), dev)
    if traj is None:
        traj = trajectory(x, y, v, fs, offsets, device)
    return _sample(ctx, x, y, v, fs, off_h, off, traj, dt, include_end)


def _poses(p, device):
    """(n, 3) poses (x, y, heading [rad]) -> three contiguous float64 device tensors"""
    t = _dev_f64(p, device).reshape(-1, 3)
    return t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2].contiguous()


def _conn_solve(ctx, f, t, radius, reversing):
    """fcpp_dubins_solve, or fcpp_rs_solve if `reversing`, on prepared poses -> (word, seg (n, 3) or (n, 5), length)"""
    torch = _torch()
    n = int(f[0].numel())
    if int(t[0].numel()) != n:
        raise ValueError('from_poses and to_poses must hold the same number of poses')
    dev = f[0].device
    word = torch.empty(n, dtype=torch.int32, device=dev)
    seg = torch.empty((n, 5 if reversing else 3), dtype=torch.float64, device=dev)
    length = torch.empty(n, dtype=torch.float64, device=dev)
    ctx.bind_stream()
    entry = ctx.lib.fcpp_rs_solve if reversing else ctx.lib.fcpp_dubins_solve
    L.check(entry(ctx.handle, n, _ptr(f[0]), _ptr(f[1]), _ptr(f[2]), _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), float(radius), _ptr(word), _ptr(seg),
                  _ptr(length)))
    return word, seg, length


def _conn_solve_poses(from_poses, to_poses, radius, reversing, device):
    ctx = get_context(device)
    dev = _torch().device('cuda', ctx.device)
    return _conn_solve(ctx, _poses(from_poses, dev), _poses(to_poses, dev), radius, reversing)


def _conn_matrix(from_poses, to_poses, radius, want_words, reversing, device):
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    f, t = _poses(from_poses, dev), _poses(to_poses, dev)
    nf, nt = int(f[0].numel()), int(t[0].numel())
    D = torch.empty((nf, nt), dtype=torch.float64, device=dev)
    W = torch.empty((nf, nt), dtype=torch.int8, device=dev) if want_words else None
    ctx.bind_stream()
    entry = ctx.lib.fcpp_rs_matrix if reversing else ctx.lib.fcpp_dubins_matrix
    L.check(entry(ctx.handle, nf, _ptr(f[0]), _ptr(f[1]), _ptr(f[2]), nt, _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), float(radius), _ptr(D), _ptr(W)))
    return (D, W) if want_words else D


def _conn_sample_solved(ctx, f, word, seg, length, radius, spacing, reversing):
    """counts + sample of SOLVED connectors that start at the prepared poses f -> dict of device tensors; `reversing` adds the samples' gear"""
    torch = _torch()
    dev = word.device
    n = int(word.numel())

    def counts(off, off_h):
        if reversing:
            return ctx.lib.fcpp_rs_counts(ctx.handle, n, _ptr(word), _ptr(seg), float(spacing), off, off_h)
        return ctx.lib.fcpp_dubins_counts(ctx.handle, n, _ptr(length), float(spacing), off, off_h)

    def fill(off, off_h, m, *cols):
        entry = ctx.lib.fcpp_rs_sample if reversing else ctx.lib.fcpp_dubins_sample
        return entry(ctx.handle, n, _ptr(f[0]), _ptr(f[1]), _ptr(f[2]), float(radius), _ptr(word), _ptr(seg), float(spacing), off, m, *cols, off_h)

    off, off_h, *cols = _counts_fill(n, dev, counts, fill, (torch.float64,) * 4 + ((torch.int8,) if reversing else ()))
    out = dict(zip(('x', 'y', 'heading', 'kappa', 'gear'), cols))          # (gear: the fifth column, with `reversing`)
    out.update(offsets=off, offsets_host=off_h, word=word, seg=seg, length=length, spacing=float(spacing))
    return out


def _conn_paths(ctx, from_poses, to_poses, radius, spacing, reversing):
    """solve + counts + sample -> dict of device tensors; `reversing` adds the samples' gear"""
    dev = _torch().device('cuda', ctx.device)
    f, t = _poses(from_poses, dev), _poses(to_poses, dev)
    word, seg, length = _conn_solve(ctx, f, t, radius, reversing)
    return _conn_sample_solved(ctx, f, word, seg, length, radius, spacing, reversing)


def _dubins_paths(ctx, from_poses, to_poses, radius, spacing):
    return _conn_paths(ctx, from_poses, to_poses, radius, spacing, False)


def _rs_paths(ctx, from_poses, to_poses, radius, spacing):
    return _conn_paths(ctx, from_poses, to_poses, radius, spacing, True)


def dubins_solve(from_poses, to_poses, radius, device=None):
    """Shortest forward-only Dubins path of every pair from_poses[i] -> to_poses[i] (fcpp_dubins_solve) for the turning radius `radius` [m].
    Poses: (n, 3) arrays or tensors (x, y, heading [rad]).  -> (word, seg, length) device tensors: the winning word (0 LSL, 1 LSR, 2 RSL,
    3 RSR, 4 RLR, 5 LRL; -1 for a pair with a non-finite input), its three segment lengths [m] (n, 3) and their sum."""
    return _conn_solve_poses(from_poses, to_poses, radius, False, device)


def dubins_matrix(from_poses, to_poses, radius, want_words=False, device=None):
    """The transit matrix D[i][j] = shortest Dubins length from exit pose i to entry pose j (fcpp_dubins_matrix): (n_from, n_to) float64 on
    the device, the layout ga_fitness / ga_evolve take when both lists are the same nodes.  Not symmetric.  want_words: also the winning
    words, (n_from, n_to) int8."""
    return _conn_matrix(from_poses, to_poses, radius, want_words, False, device)


def dubins_paths(from_poses, to_poses, radius, spacing, device=None):
    """The shortest Dubins paths of the pairs, sampled every `spacing` metres (fcpp_dubins_solve + _counts + _sample) -> (x, y, heading, kappa,
    offsets) device tensors: path p owns the samples offsets[p] .. offsets[p + 1]; its first sample is its start pose, sample k lies at arc
    length k * spacing, its last sample is the path's end.  kappa: +1/radius on left arcs, -1/radius on right arcs, 0 on the straight."""
    o = _dubins_paths(get_context(device), from_poses, to_poses, radius, spacing)
    return o['x'], o['y'], o['heading'], o['kappa'], o['offsets']


def rs_solve(from_poses, to_poses, radius, device=None):
    """Shortest Reeds-Shepp path (forward and reverse motion) of every pair from_poses[i] -> to_poses[i] (fcpp_rs_solve) for the turning
    radius `radius` [m].  Poses: (n, 3) arrays or tensors (x, y, heading [rad]).  -> (word, seg, length) device tensors: the winning word
    (0 .. 47, the table of include/fcpp.h: 4 * base + flip + 2 * mirror; -1 for a pair with a non-finite input), its five SIGNED segment
    lengths [m] (n, 5) -- positive forward, negative reverse, unused ones 0 -- and the sum of their magnitudes."""
    return _conn_solve_poses(from_poses, to_poses, radius, True, device)


def rs_matrix(from_poses, to_poses, radius, want_words=False, device=None):
    """The transit matrix of a vehicle that reverses: D[i][j] = shortest Reeds-Shepp length from pose i to pose j (fcpp_rs_matrix),
    (n_from, n_to) float64 on the device, the layout ga_fitness / ga_evolve take.  A metric: symmetric (to rounding) when both lists are
    the same poses, with a zero diagonal.  want_words: also the winning words, (n_from, n_to) int8."""
    return _conn_matrix(from_poses, to_poses, radius, want_words, True, device)


def rs_paths(from_poses, to_poses, radius, spacing, device=None):
    """The shortest Reeds-Shepp paths of the pairs, sampled every `spacing` metres PER GEAR RUN (fcpp_rs_solve + _counts + _sample) ->
    (x, y, heading, kappa, gear, offsets) device tensors: path p owns the samples offsets[p] .. offsets[p + 1]; its first sample is its start
    pose, its last the goal; within a run sample k lies k * spacing from the run's start and the run's last sample is its end, so every cusp
    appears twice, with the same pose and the opposite gear.  heading: the vehicle's (against the motion in reverse); gear: int8 +1 / -1."""
    o = _rs_paths(get_context(device), from_poses, to_poses, radius, spacing)
    return o['x'], o['y'], o['heading'], o['kappa'], o['gear'], o['offsets']


# ---- swaths of any polygon field (fcpp_swath_scores / _counts / _fill; the rule: include/fcpp.h) --------------------------------------
@dataclass
class PolygonFields:
    """polygon_fields(): n fields as the two-level CSR of the library, on the device"""
    ring_offsets: object        # (n + 1) int64: fields -> rings
    vert_offsets: object        # (n_rings + 1) int64: rings -> vertices
    x: object                   # (n_verts) float64
    y: object

    @property
    def n(self):
        return int(self.ring_offsets.numel()) - 1

    def _head(self):
        return (self.n, _ptr(self.ring_offsets), int(self.vert_offsets.numel()) - 1, _ptr(self.vert_offsets), int(self.x.numel()), _ptr(self.x),
                _ptr(self.y))


def _rings(field):
    if isinstance(field, np.ndarray) and field.ndim == 2:
        return [field]
    field = list(field)
    if field and np.ndim(field[0]) == 1 and len(field[0]) == 2 and np.ndim(field[0][0]) == 0:
        return [field]                 # one ring given as a vertex list
    return field


def polygon_fields(fields, device=None):
    """Pack a list of fields for the swath operators.  A field is an (m, 2) array of vertices (one ring) or a list of rings, ring 0 the outer
    boundary and further rings holes; rings are closed implicitly and may have either orientation (even-odd interior).  The swath operators take the
    WORK AREA: headland() makes it from a surveyed boundary (polygon_inset at the headland's width).  -> PolygonFields on the device (a
    PolygonFields is returned as it is)."""
    if isinstance(fields, PolygonFields):
        return fields
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    ro, vo, xy = [0], [0], []
    for f in fields:
        for r in _rings(f):
            r = np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r, dtype=np.float64).reshape(-1, 2)
            xy.append(r)
            vo.append(vo[-1] + len(r))
        ro.append(len(vo) - 1)
    xy = np.concatenate(xy) if xy else np.zeros((0, 2))
    return PolygonFields(torch.as_tensor(np.asarray(ro, dtype=np.int64), device=dev), torch.as_tensor(np.asarray(vo, dtype=np.int64), device=dev),
                         torch.as_tensor(np.ascontiguousarray(xy[:, 0]), device=dev), torch.as_tensor(np.ascontiguousarray(xy[:, 1]), device=dev))


# ---- headland passes of any polygon field (fcpp_inset_counts / _fill; the rule: include/fcpp.h) -----------------------------------------
@dataclass
class InsetSet:
    """polygon_inset(): the insets of n fields at D distances.  Pair (i, j) = i D + j owns the rings pair_ring_offsets[p] .. [p + 1] and the
    vertices pair_vert_offsets[p] .. [p + 1]; ring r owns the vertices ring_offsets[r] .. [r + 1].  Rings are closed implicitly, the kept
    area on their left (outer boundaries counter-clockwise, grown holes clockwise)."""
    n: int
    distances: object                   # (D) float64, device
    pair_ring_offsets: object           # (n D + 1) int64, device; *_host: the numpy copies
    pair_ring_offsets_host: object
    pair_vert_offsets: object           # (n D + 1) int64
    pair_vert_offsets_host: object
    ring_offsets: object                # (n_rings + 1) int64: rings -> vertices
    x: object                           # (n_verts) float64
    y: object
    src: object                         # (n_verts) int32: the primitive that emitted the vertex, 2 g (edge g's offset) or 2 g + 1 (the arc behind it)
    status: object                      # (n, D) int32
    gap: object                         # (n, D) float64: the largest distance between joined pieces [m]

    @property
    def D(self):
        return int(self.distances.numel())

    def rings(self, i, j):
        """the rings of field i at distance j: a list of (m, 2) device tensors"""
        torch = _torch()
        p = i * self.D + j
        r0, r1 = int(self.pair_ring_offsets_host[p]), int(self.pair_ring_offsets_host[p + 1])
        off = self.ring_offsets[r0:r1 + 1].cpu().numpy()
        return [torch.stack([self.x[off[k]:off[k + 1]], self.y[off[k]:off[k + 1]]], dim=1) for k in range(r1 - r0)]

    def as_fields(self, j):
        """the inset of every field at distance j as PolygonFields (a field whose inset is empty, or whose status is non-zero, has no
        ring there): gathered on the device from the CSR arrays; only the sizes come from the host copies of the offsets"""
        torch = _torch()
        dev = self.x.device
        D = self.D
        pro_h, pvo_h = self.pair_ring_offsets_host, self.pair_vert_offsets_host
        pairs = np.arange(self.n, dtype=np.int64) * D + j
        n_r, n_v = pro_h[pairs + 1] - pro_h[pairs], pvo_h[pairs + 1] - pvo_h[pairs]
        R, V = int(n_r.sum()), int(n_v.sum())
        ring_off = torch.as_tensor(np.concatenate([[0], np.cumsum(n_r)]).astype(np.int64), device=dev)
        pd = torch.as_tensor(pairs, device=dev)
        cnt_r = self.pair_ring_offsets[pd + 1] - self.pair_ring_offsets[pd]
        first_r = torch.repeat_interleave(self.pair_ring_offsets[pd] - ring_off[:-1], cnt_r, output_size=R)
        rid = first_r + torch.arange(R, dtype=torch.int64, device=dev)                  # the rings, in field order
        cnt_v = self.ring_offsets[rid + 1] - self.ring_offsets[rid]
        vert_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
        vert_off[1:] = torch.cumsum(cnt_v, dim=0)
        first_v = torch.repeat_interleave(self.ring_offsets[rid] - vert_off[:-1], cnt_v, output_size=V)
        vid = first_v + torch.arange(V, dtype=torch.int64, device=dev)
        return PolygonFields(ring_off, vert_off, self.x[vid].contiguous(), self.y[vid].contiguous())


def polygon_inset(fields, distances, arc_step=0.1, device=None):
    """The inset (fcpp_inset_counts + fcpp_inset_fill): for every field and every distance d [m] of `distances` the boundary of the set of
    points inside the field that lie at least d from its boundary -- offset edges, and arcs of radius d around reflex vertices drawn as
    inscribed chords of at most arc_step rad.  The inset may consist of several rings, a hole may merge with the outer boundary, the inset
    may be empty (0 rings, status 0).  status: 0, FCPP_EINVAL or FCPP_EUNSUPPORTED (more than 1024 edges, a critical distance); such a pair
    has no rings.  -> InsetSet."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    pf = polygon_fields(fields, device)
    dist = _dev_f64(distances, dev).reshape(-1)
    n, D = pf.n, int(dist.numel())
    m = n * D
    args = (*pf._head(), D, _ptr(dist), float(arc_step))
    pro, pvo = torch.empty(m + 1, dtype=torch.int64, device=dev), torch.empty(m + 1, dtype=torch.int64, device=dev)
    pro_h, pvo_h = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    st, gap = torch.zeros((n, D), dtype=torch.int32, device=dev), torch.zeros((n, D), dtype=torch.float64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_inset_counts(ctx.handle, *args, _ptr(pro), _host_ptr(pro_h), _ptr(pvo), _host_ptr(pvo_h), _ptr(st), _ptr(gap)))
    R, V = int(pro_h[-1]), int(pvo_h[-1])
    ovo = torch.empty(R + 1, dtype=torch.int64, device=dev)
    x, y = torch.empty(V, dtype=torch.float64, device=dev), torch.empty(V, dtype=torch.float64, device=dev)
    src = torch.empty(V, dtype=torch.int32, device=dev)
    L.check(ctx.lib.fcpp_inset_fill(ctx.handle, *args, _ptr(pro), _ptr(pvo), R, V, _ptr(ovo), _ptr(x), _ptr(y), _ptr(src)))
    return InsetSet(n, dist, pro, pro_h, pvo, pvo_h, ovo, x, y, src, st, gap)


def headland(fields, width, passes, first=None, arc_step=0.1, device=None):
    """The headland of every field: `passes` >= 1 passes of working width `width` along the boundary (holes included), and what they leave.
    -> (InsetSet, PolygonFields): the centre lines of passes k = 1 .. passes, the inset at first + (k - 1) width (first: default width / 2),
    as column k - 1 of the InsetSet; and the work area, the inset at passes x width, which swath_scores, best_swath_angle, polygon_swaths
    and route_swaths accept as it is.  A field whose work area is empty has no ring there: the swath operators report it as FCPP_EINVAL per
    field, as they do any field without a ring, and plan the rest."""
    passes = int(passes)
    if passes < 1:
        raise ValueError('passes must be at least 1')
    pf = polygon_fields(fields, device)
    f0 = float(width) / 2 if first is None else float(first)
    lines = polygon_inset(pf, [f0 + k * float(width) for k in range(passes)], arc_step, device)
    work = polygon_inset(pf, [passes * float(width)], arc_step, device)
    return lines, work.as_fields(0)


def _first(width, first):
    return float(width) / 2 if first is None else float(first)


def swath_scores(fields, angles, width, first=None, min_length=0.0, device=None):
    """The angle search (fcpp_swath_scores): every field cut at every track angle of `angles` [rad] into parallel tracks of working width
    `width`; line 0 lies `first` (default width / 2) above the field's lowest point across the tracks; pieces no longer than min_length are
    dropped.  -> (n_swaths, n_lines, length, status) device tensors of shape (n, A): swath count, line count, summed swath length [m] and
    status (0, FCPP_EINVAL or FCPP_EUNSUPPORTED: such a pair has zeros) of field i at angles[j]."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    pf = polygon_fields(fields, device)
    ang = _dev_f64(angles, dev).reshape(-1)
    n, A = pf.n, int(ang.numel())
    n_sw, n_ln, st = (torch.zeros((n, A), dtype=torch.int32, device=dev) for _ in range(3))
    length = torch.zeros((n, A), dtype=torch.float64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_swath_scores(ctx.handle, *pf._head(), A, _ptr(ang), float(width), _first(width, first), float(min_length), _ptr(n_sw),
                                      _ptr(n_ln), _ptr(length), _ptr(st)))
    return n_sw, n_ln, length, st


def best_swath_angle(fields, angles, width, turn_cost=0.0, first=None, min_length=0.0, device=None):
    """For every field the index into `angles` that minimises length + turn_cost * n_swaths (swath_scores; the argmin is torch's, on the
    device), ties to the lowest index; -1 for a field whose status is non-zero at every angle.  -> (index (n,) int64, cost (n, A))."""
    torch = _torch()
    n_sw, _, length, st = swath_scores(fields, angles, width, first, min_length, device)
    cost = torch.where(st == 0, length + float(turn_cost) * n_sw.to(torch.float64), torch.full_like(length, float('inf')))
    if cost.shape[1] == 0:
        return torch.full((cost.shape[0],), -1, dtype=torch.int64, device=cost.device), cost
    # the first index that attains the minimum (argmin alone does not promise which of equal entries it returns)
    idx = (cost == cost.min(dim=1, keepdim=True).values).to(torch.int8).argmax(dim=1)
    return torch.where((st == 0).any(dim=1), idx, torch.full_like(idx, -1)), cost


@dataclass
class SwathSet:
    """polygon_swaths(): the swaths of n fields.  Field i owns the records offsets[i] .. offsets[i + 1], ordered by line, then along it."""
    offsets: object             # (n + 1) int64, device; offsets_host: the numpy copy
    offsets_host: object
    a: object                   # (m, 2) float64: the end point with the smaller coordinate along the tracks
    b: object                   # (m, 2)
    line: object                # (m) int32: the line index k of the swath
    length: object              # (m) float64
    status: object              # (n) int32
    n_lines: object             # (n) int32
    angle: object               # (n) float64: the track angle of every field

    def poses(self, i):
        """field i's swaths as poses (x, y, heading): (start, end) driven from a to b -- heading theta -- and (start, end) driven the other
        way, from b to a with heading theta + pi; each (m_i, 3), ready for dubins_matrix / rs_matrix"""
        torch = _torch()
        sl = slice(int(self.offsets_host[i]), int(self.offsets_host[i + 1]))
        a, b = self.a[sl], self.b[sl]
        th = self.angle[i].expand(a.shape[0], 1)
        fwd = (torch.cat([a, th], dim=1), torch.cat([b, th], dim=1))
        return fwd, (torch.cat([b, th + np.pi], dim=1), torch.cat([a, th + np.pi], dim=1))


def polygon_swaths(fields, angle, width, first=None, min_length=0.0, device=None):
    """The cut (fcpp_swath_counts + fcpp_swath_fill): every field's swaths at its track angle -- `angle` is a scalar or one value per field.
    Parameters as for swath_scores.  -> SwathSet."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    pf = polygon_fields(fields, device)
    n = pf.n
    ang = _one_per(_dev_f64(angle, dev), n, 'angle', 'value per field')
    args = (*pf._head(), _ptr(ang), float(width), _first(width, first), float(min_length))
    off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    off_h = np.zeros(n + 1, dtype=np.int64)
    n_ln, st = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_swath_counts(ctx.handle, *args, _ptr(off), _host_ptr(off_h), _ptr(n_ln), _ptr(st)))
    m = int(off_h[-1])
    a, b = torch.empty((2, m), dtype=torch.float64, device=dev), torch.empty((2, m), dtype=torch.float64, device=dev)
    line, length = torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.float64, device=dev)
    L.check(ctx.lib.fcpp_swath_fill(ctx.handle, *args, _ptr(off), m, _ptr(a[0]), _ptr(a[1]), _ptr(b[0]), _ptr(b[1]), _ptr(line), _ptr(length)))
    return SwathSet(off, off_h, a.t().contiguous(), b.t().contiguous(), line, length, st, n_ln, ang)


def _chord_radius(radius, spacing):
    """The radius R' >= radius of an arc whose polyline, sampled every `spacing` metres, has the chord curvature 1 / radius: curvature()
    is the chord formula (turning angle of two chords over their mean length), which on an arc of radius R' gives (1/R') x / sin x with
    x = spacing / (2 R'), ABOVE 1/R'.  So R' = radius * x / sin x, a fixed point reached in a few steps (x / sin x = 1 + x^2/6 + ..)."""
    R, h = float(radius), float(spacing) / 2
    for _ in range(50):
        x = h / R
        nxt = float(radius) * x / np.sin(x) if x > 0.0 else float(radius)
        if nxt == R:
            break
        R = nxt
    return R


def swath_route(swathset, i, radius, spacing, reversing=False, device=None, order=None):
    """The route of field i of a SwathSet.  order=None: the plain boustrophedon route, its swaths in their STORED order (by line, then along
    the line), driven in alternating directions; order = an int array of oriented swaths (2 s + d: swath s of the field, d = 0 from a to b,
    d = 1 from b to a, every swath once) or a SwathRoute of the same SwathSet (route_swaths): the swaths in that order and those directions.
    Each swath is sampled every `spacing` metres (its last sample is its end), and consecutive swaths are joined by the shortest
    Dubins path -- Reeds-Shepp if `reversing` -- from the end pose of one to the start pose of the next (dubins_paths / rs_paths).
    `radius` is the vehicle's least turning radius.  The connectors are planned with the slightly larger radius at which the SAMPLED
    polyline turns no tighter than 1 / radius by the project's own measure, curvature() (_chord_radius: + 0.016 % at radius 8 and spacing
    0.5), so the route passes speed_plan's curvature clamp untouched; at a cusp of a reversing connector the chord formula sees a turn on
    the spot, as on every Reeds-Shepp path.  -> (x, y, heading, part) device tensors; part (int8) is 0 on a swath and 1 on a connector.
    The stored order is NOT optimised, whatever the shape of the field: route_swaths chooses an order and directions (pass it the same
    `spacing`, so that it prices the connectors driven here).  A connector is the shortest path between two poses and knows no boundary
    unless `clear_of` is given to route_swaths: it may leave the field or cross a hole; validate() (fcpp_validate) flags that, as for every
    connector of this library, and connector_clearance tests it exactly."""
    torch = _torch()
    (f_s, f_e), (r_s, r_e) = swathset.poses(i)
    m = int(f_s.shape[0])
    dev = f_s.device
    if m == 0:
        e = torch.empty(0, dtype=torch.float64, device=dev)
        return e, e.clone(), e.clone(), torch.empty(0, dtype=torch.int8, device=dev)
    length = swathset.length[int(swathset.offsets_host[i]):int(swathset.offsets_host[i + 1])]
    if order is None:
        odd = (torch.arange(m, device=dev) % 2 == 1).unsqueeze(1)
        start, end = torch.where(odd, r_s, f_s), torch.where(odd, r_e, f_e)
    else:
        o = order.field(i) if isinstance(order, SwathRoute) else order
        o = torch.as_tensor(o, device=dev).to(torch.int64).reshape(-1)
        idx = o >> 1
        if int(o.numel()) != m or not torch.equal(torch.sort(idx).values, torch.arange(m, device=dev)):
            raise ValueError('order must hold every swath of the field exactly once, as 2 * swath + direction')
        odd = (o & 1).to(torch.bool).unsqueeze(1)
        start, end = torch.where(odd, r_s[idx], f_s[idx]), torch.where(odd, r_e[idx], f_e[idx])
        length = length[idx]
    con = None
    if m > 1:
        con = _conn_paths(get_context(device), end[:-1], start[1:], _chord_radius(radius, spacing), spacing, reversing)
    c_off = con['offsets_host'] if con is not None else None
    length = length.cpu().numpy()
    xs, ys, hs, parts = [], [], [], []
    for j in range(m):
        K = int(np.floor(length[j] / float(spacing))) + 1
        t = torch.arange(K, dtype=torch.float64, device=dev) * float(spacing)
        if (K - 1) * float(spacing) < length[j]:
            t = torch.cat([t, swathset.length.new_tensor([length[j]])])
        t = (t / length[j]).clamp(max=1.0)
        x = start[j, 0] + t * (end[j, 0] - start[j, 0])
        y = start[j, 1] + t * (end[j, 1] - start[j, 1])
        x[-1], y[-1] = end[j, 0], end[j, 1]
        xs.append(x); ys.append(y); hs.append(start[j, 2].expand(x.numel())); parts.append(torch.zeros(x.numel(), dtype=torch.int8, device=dev))
        if j + 1 < m:
            sl = slice(int(c_off[j]), int(c_off[j + 1]))
            xs.append(con['x'][sl]); ys.append(con['y'][sl]); hs.append(con['heading'][sl])
            parts.append(torch.ones(sl.stop - sl.start, dtype=torch.int8, device=dev))
    return torch.cat(xs), torch.cat(ys), torch.cat(hs), torch.cat(parts)


# ---- the swath router (fcpp_route_transit / fcpp_route_solve; the rule: include/fcpp.h) ----------------------------------------------------
ROUTE_T_BUDGET = 1 << 30         # bytes of transit blocks one call of the library holds: route_swaths solves the fields in chunks below it


@dataclass
class SwathRoute:
    """route_swaths(): for every field of a SwathSet the order and directions in which to drive its swaths.  Field i owns
    order[offsets_host[i] : offsets_host[i + 1]] (the SwathSet's offsets): oriented swaths 2 s + d in driving order, s the swath's index
    within the field, d = 0 from a to b, d = 1 from b to a."""
    offsets_host: object        # (n + 1) int64, numpy
    order: object               # (m) int32, device
    cost: object                # (n) float64: the summed connector lengths of `order` [m] (with the entry / exit connectors, if given)
    stored_cost: object         # (n) float64: the same for the stored boustrophedon order, what swath_route drives without an order
    winner: object              # (n) int32: the candidate that gave `order`
    sweeps: object              # (n) int32: the most moves any candidate of the field applied
    status: object              # (n) int32: 0, FCPP_EUNSUPPORTED (more than 512 swaths) or FCPP_EINVAL (a non-finite cost): the stored order
    tours: object               # (starts, m) int32: every candidate's final tour
    costs: object               # (n, starts) float64: and its cost
    blocked: object = None      # with clear_of: (n) int32, the connectors of `order` AS DRIVEN that are not clear, entry and exit included
    blocked_stored: object = None       # with clear_of: the same for the stored boustrophedon order
    length: object = None       # with clear_of: (n) float64, the summed connector lengths of `order` without any penalty [m]
    clearance: object = None    # with clear_of: the FieldPathClearance behind `blocked` and `length`: every connector of `order`, leg by leg
    reshaped: object = None     # with price_clear: (n) int32, the connectors of `order` whose clear word is not the shortest one (rank > 0)

    def field(self, i):
        return self.order[int(self.offsets_host[i]):int(self.offsets_host[i + 1])]


def _route_offsets(soff_h):
    """the transit block offsets of fields with these swath offsets: block i is (2 m_i)^2 entries, none beyond the cap"""
    m = np.diff(soff_h)
    toff = np.zeros(len(soff_h), dtype=np.int64)
    np.cumsum(np.where(m > L.ROUTE_MAX_SWATHS, 0, 4 * m * m), out=toff[1:])
    return toff


@dataclass
class _RouteChunk:
    """fields lo .. hi of a SwathSet as the router's entries take them, with offsets of the chunk's own; built once per chunk"""
    soff: object                # (hi - lo + 1) int64, device: the chunk's swath offsets; soff_h: the numpy copy
    soff_h: object
    toff: object                # (hi - lo + 1) int64, device: its transit block offsets (_route_offsets); toff_h: the numpy copy
    toff_h: object
    ends: object                # ax, ay, bx, by: the swaths' end points as four contiguous columns
    ang: object                 # (hi - lo) float64: the fields' track angles
    m: int                      # the chunk's swaths

    @classmethod
    def of(cls, ss, lo, hi):
        torch = _torch()
        dev = ss.a.device
        s0, s1 = int(ss.offsets_host[lo]), int(ss.offsets_host[hi])
        soff_h = np.ascontiguousarray(ss.offsets_host[lo:hi + 1] - s0, dtype=np.int64)
        toff_h = _route_offsets(soff_h)
        ends = tuple(t[s0:s1, k].contiguous() for t in (ss.a, ss.b) for k in (0, 1))
        return cls(torch.as_tensor(soff_h, device=dev), soff_h, torch.as_tensor(toff_h, device=dev), toff_h, ends, ss.angle[lo:hi].contiguous(), s1 - s0)

    def block(self, dtype):
        """an unwritten tensor of the transit blocks' layout"""
        return _torch().empty(int(self.toff_h[-1]), dtype=dtype, device=self.soff.device)

    def head(self, radius, reversing):
        """the arguments the three transit entries share, behind the handle"""
        return (len(self.soff_h) - 1, _ptr(self.soff), _host_ptr(self.soff_h), self.m, *[_ptr(t) for t in self.ends], _ptr(self.ang), float(radius),
                1 if reversing else 0, _ptr(self.toff), _host_ptr(self.toff_h), int(self.toff_h[-1]))


def _route_transit(ctx, ch, radius, reversing):
    """fcpp_route_transit on a _RouteChunk -> T: its transit blocks"""
    T = ch.block(_torch().float64)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_route_transit(ctx.handle, *ch.head(radius, reversing), _ptr(T)))
    return T


def _route_chunks(soff_h, budget):
    """[lo, hi) ranges of consecutive fields whose transit blocks stay within `budget` bytes (a field alone is at most 8 MiB)"""
    size = np.diff(_route_offsets(soff_h)) * 8
    out, lo, acc = [], 0, 0
    for i, b in enumerate(size):
        if i > lo and acc + b > budget:
            out.append((lo, i))
            lo, acc = i, 0
        acc += int(b)
    if len(size) > lo or not out:
        out.append((lo, len(size)))
    return out


def _fields_slice(pf, ro_h, vo_h, lo, hi):
    """fields lo .. hi of a PolygonFields as one of their own (ro_h, vo_h: host copies of its two offset arrays)"""
    if lo == 0 and hi == pf.n:
        return pf
    r0, r1 = int(ro_h[lo]), int(ro_h[hi])
    v0, v1 = int(vo_h[r0]), int(vo_h[r1])
    return PolygonFields((pf.ring_offsets[lo:hi + 1] - r0).contiguous(), (pf.vert_offsets[r0:r1 + 1] - v0).contiguous(), pf.x[v0:v1].contiguous(),
                         pf.y[v0:v1].contiguous())


def _route_transit_clear(ctx, ch, radius, reversing, pf, penalty, T):
    """fcpp_route_transit_clear on the chunk whose blocks T _route_transit made: T in / out -> B (uint8, T's layout); pf: the chunk's own
    fields"""
    B = ch.block(_torch().uint8)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_route_transit_clear(ctx.handle, *ch.head(radius, reversing), *pf._head()[1:], float(penalty), _ptr(T), _ptr(B)))
    return B


def _route_transit_priced(ctx, ch, radius, reversing, pf, penalty):
    """fcpp_route_transit_priced on a _RouteChunk -> (T, K): its PRICED transit blocks (T out only) and K (int8, T's layout); pf: the chunk's
    own fields"""
    torch = _torch()
    T, K = ch.block(torch.float64), ch.block(torch.int8)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_route_transit_priced(ctx.handle, *ch.head(radius, reversing), *pf._head()[1:], float(penalty), _ptr(T), _ptr(K)))
    return T, K


def _clear_fields(clear_of, n, device):
    pf = polygon_fields(clear_of, device)
    if pf.n != n:
        raise ValueError('clear_of must hold one field per field of the SwathSet')
    return pf


def swath_transit(swathset, radius, reversing=False, device=None, clear_of=None, blocked_penalty=1.0e6, price_clear=False):
    """The transit blocks of every field of a SwathSet (fcpp_route_transit) -> (T, offsets): T a flat float64 device tensor, field i's block
    T[offsets[i] : offsets[i + 1]].reshape(2 m_i, 2 m_i) (offsets: numpy int64), entry [p][q] the shortest Dubins -- Reeds-Shepp if
    `reversing` -- length from the end of oriented swath p to the start of oriented swath q (p = 2 s + d: swath s from a to b for d = 0, from
    b to a for d = 1), +inf within one swath; [p][q] and [q ^ 1][p ^ 1] hold equal bits.  A field of more than 512 swaths has no block.
    clear_of (one field per field of the SwathSet, as polygon_fields takes them): every connector is also tested against its field
    (fcpp_route_transit_clear; the rule: include/fcpp.h) -> (T, offsets, B): B uint8 with T's layout, 1 where the connector is not clear,
    and there T holds length + blocked_penalty.  The default penalty of 1e6 m is a condition, not a measurement: it lies beyond any
    route's transit total (512 swaths at field-diameter transits stay far below it), so one blocked connector outweighs every order
    without one; and it is small enough that a delta of three penalised entries (3e6, ulp 4.7e-10) still resolves the router's min_gain
    of 1e-9 m in double.  blocked_penalty = 0 reports B and leaves T as it is.
    price_clear=True (with clear_of; ValueError without): the PRICED blocks (fcpp_route_transit_priced) -> (T, offsets, K): every transit
    holds the length of the shortest word that is clear of its field -- what clear_connectors and field_paths(clear_of=...) drive for the
    pair -- and K (int8, T's layout) that word's rank; where no word is clear K is -1 and T the shortest length + blocked_penalty."""
    if price_clear and clear_of is None:
        raise ValueError('price_clear=True needs clear_of: the region the connectors have to stay clear of')
    ctx = get_context(device)
    n = len(swathset.offsets_host) - 1
    ch = _RouteChunk.of(swathset, 0, n)
    if price_clear:
        T, K = _route_transit_priced(ctx, ch, radius, reversing, _clear_fields(clear_of, n, device), blocked_penalty)
        return T, ch.toff_h, K
    T = _route_transit(ctx, ch, radius, reversing)
    if clear_of is None:
        return T, ch.toff_h
    return T, ch.toff_h, _route_transit_clear(ctx, ch, radius, reversing, _clear_fields(clear_of, n, device), blocked_penalty, T)


def _route_end_pairs(ss, pose, at_entry):
    """the pairs behind E (at_entry) or X of route_swaths: each field's pose and every oriented swath's start / end -> (from, to), (2 m, 3)"""
    torch = _torch()
    dev = ss.a.device
    pose = _dev_f64(pose, dev).reshape(-1, 3)
    counts = torch.as_tensor(np.diff(ss.offsets_host), device=dev)
    if pose.shape[0] != counts.numel():
        raise ValueError('entry / exit must hold one pose (x, y, heading) per field')
    th = torch.repeat_interleave(ss.angle, counts).unsqueeze(1)
    # oriented swath 2 s starts at a and ends at b with heading theta, 2 s + 1 starts at b and ends at a with theta + pi (SwathSet.poses)
    first, second = (ss.a, ss.b) if at_entry else (ss.b, ss.a)
    own = torch.stack([torch.cat([first, th], dim=1), torch.cat([second, th + np.pi], dim=1)], dim=1).reshape(-1, 3)
    far = torch.repeat_interleave(pose, 2 * counts, dim=0)
    return (far, own) if at_entry else (own, far)


def _route_ends(ss, pose, at_entry, radius, reversing, device, clear_of=None, penalty=0.0, price_clear=False):
    """E (at_entry) or X of route_swaths: the connector length between each field's pose and every oriented swath's start / from its end;
    clear_of (PolygonFields): + penalty where that connector is not clear of its field; price_clear: the shortest clear word's length
    (clear_connectors), + penalty where no word is clear"""
    torch = _torch()
    frm, to = _route_end_pairs(ss, pose, at_entry)
    if clear_of is None:
        return _conn_solve_poses(frm, to, radius, reversing, device)[2].contiguous()
    pair_field = _owners(2 * ss.offsets, 2 * int(ss.offsets_host[-1]))
    if price_clear:
        c = clear_connectors(frm, to, clear_of, pair_field, radius, reversing, device)
        return torch.where(c.rank < 0, c.length + float(penalty), c.length).contiguous()
    c = _connector_clearance(frm, to, clear_of, pair_field, radius, reversing, device)
    return torch.where(c.clear, c.length, c.length + float(penalty)).contiguous()


def route_swaths(swathset, radius, reversing=False, entry=None, exit=None, starts=8, min_gain=1e-9, max_sweeps=None, spacing=None, device=None,
                 clear_of=None, blocked_penalty=1.0e6, price_clear=False):
    """Order and direction of every field's swaths (fcpp_route_transit + fcpp_route_solve; the rule: include/fcpp.h) -> SwathRoute.
    The cost of a tour is the summed length of its connectors -- shortest Dubins paths at the turning radius `radius`, Reeds-Shepp if
    `reversing` -- plus, with entry / exit (one pose (x, y, heading) per field, or None), the connector from the field's entry pose to
    the first swath and from the last swath to its exit pose.  `starts` candidate tours per field (the stored boustrophedon, its mirror,
    nearest-neighbour tours from spread starts) are each improved by segment reversals and or-opt moves until none gains more than
    min_gain [m] (or max_sweeps moves: None = 8 x the largest swath count + 8); the cheapest wins.  spacing: plan at the radius swath_route
    drives its connectors with at that sample spacing (_chord_radius), so `cost` is the length swath_route(order=...) drives.  Connectors
    know no boundary (validate() flags what leaves the field) unless `clear_of` is given.  Fields are solved in chunks of at most
    ROUTE_T_BUDGET bytes of transit blocks.  A field of more than 512 swaths keeps its stored order (status FCPP_EUNSUPPORTED).
    clear_of (one field per field of the SwathSet, as polygon_fields takes them -- the surveyed boundary with its ponds, say, while the
    swaths lie in its inset): every transit, entry and exit connector that is not clear of its field (fcpp_route_transit_clear,
    fcpp_conn_clear; the rule: include/fcpp.h) is priced at length + blocked_penalty (swath_transit explains the default), so the order
    avoids blocked connectors where another order can; no connector is re-shaped.  `cost` stays what the solver returned, penalties
    included; SwathRoute.length is the order's summed connector length without them, SwathRoute.blocked / blocked_stored count the
    connectors of the order / of the stored boustrophedon that are still not clear (field_path_clearance says which).  They are counted
    on the connectors AS DRIVEN: a block entry holds its canonical pair's connector, and where two words tie in length the connector
    driven for the mirrored entry may be the other one.
    price_clear=True (with clear_of; ValueError without): every transit, entry and exit connector is priced at the length of the SHORTEST
    CLEAR word of its pair (fcpp_route_transit_priced, clear_connectors) -- the word field_paths(clear_of=...) drives for it -- and at the
    shortest length + blocked_penalty only where no word is clear: the router optimises the path that is driven with reshaping.
    SwathRoute.length and .blocked are then those of the clear words as driven (clear_connectors on the legs' poses: blocked counts rank
    -1), SwathRoute.reshaped counts the legs of rank > 0; .clearance and .blocked_stored keep their meaning, the shortest words tested."""
    if price_clear and clear_of is None:
        raise ValueError('price_clear=True needs clear_of: the region the connectors have to stay clear of')
    ctx = get_context(device)
    torch = _torch()
    ss = swathset
    dev = ss.a.device
    R = float(radius) if spacing is None else _chord_radius(radius, spacing)
    soff_all = np.asarray(ss.offsets_host, dtype=np.int64)
    n, m_all = len(soff_all) - 1, np.diff(soff_all)
    S = int(starts)
    if max_sweeps is None:
        fit = m_all[m_all <= L.ROUTE_MAX_SWATHS]
        max_sweeps = min(8 * int(fit.max() if fit.size else 0) + 8, 1 << 20)
    pf = ro_h = vo_h = None
    if clear_of is not None:
        pf = _clear_fields(clear_of, n, device)
        ro_h, vo_h = pf.ring_offsets.cpu().numpy(), pf.vert_offsets.cpu().numpy()
    E_all = _route_ends(ss, entry, True, R, reversing, device, pf, blocked_penalty, price_clear) if entry is not None else None
    X_all = _route_ends(ss, exit, False, R, reversing, device, pf, blocked_penalty, price_clear) if exit is not None else None
    order = torch.empty(int(soff_all[-1]), dtype=torch.int32, device=dev)
    tours = torch.empty((max(S, 0), int(soff_all[-1])), dtype=torch.int32, device=dev)
    costs = torch.empty((n, max(S, 0)), dtype=torch.float64, device=dev)
    cost, stored = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    winner, sweeps, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    for lo, hi in _route_chunks(soff_all, ROUTE_T_BUDGET):
        ch = _RouteChunk.of(ss, lo, hi)
        m = ch.m
        if price_clear:
            T, _ = _route_transit_priced(ctx, ch, R, reversing, _fields_slice(pf, ro_h, vo_h, lo, hi), blocked_penalty)
        else:
            T = _route_transit(ctx, ch, R, reversing)
            if pf is not None:
                _route_transit_clear(ctx, ch, R, reversing, _fields_slice(pf, ro_h, vo_h, lo, hi), blocked_penalty, T)
        s0 = int(soff_all[lo])
        Ec = E_all[2 * s0:2 * (s0 + m)] if E_all is not None else None
        Xc = X_all[2 * s0:2 * (s0 + m)] if X_all is not None else None
        tr = torch.empty((max(S, 0), m), dtype=torch.int32, device=dev)
        L.check(ctx.lib.fcpp_route_solve(ctx.handle, hi - lo, _ptr(ch.soff), _host_ptr(ch.soff_h), m, _ptr(ch.toff), _host_ptr(ch.toff_h),
                                         int(ch.toff_h[-1]), _ptr(T), _ptr(Ec), _ptr(Xc), S, float(min_gain), int(max_sweeps), _ptr(tr),
                                         _ptr(costs[lo:hi]), _ptr(order[s0:s0 + m]), _ptr(cost[lo:hi]), _ptr(winner[lo:hi]), _ptr(sweeps[lo:hi]),
                                         _ptr(status[lo:hi]), _ptr(stored[lo:hi])))
        tours[:, s0:s0 + m] = tr
    route = SwathRoute(soff_all, order, cost, stored, winner, sweeps, status, tours, costs)
    if pf is not None:
        driven = _legs_clearance(ss, pf, R, reversing, order, entry, exit, device)
        route.blocked, route.length, route.clearance = driven.blocked, driven.length, driven
        route.blocked_stored = _legs_clearance(ss, pf, R, reversing, None, entry, exit, device).blocked
    if price_clear:
        frm, to, lf, _ = _leg_pairs(ss, order, entry, exit)
        c = clear_connectors(frm, to, pf, lf, R, reversing, device)
        per_field = torch.bincount(lf, minlength=n)
        route.blocked, route.reshaped = (torch.zeros(n, dtype=torch.int32, device=dev).index_add_(0, lf, w.to(torch.int32))
                                         for w in (c.rank < 0, c.rank > 0))
        route.length = torch.segment_reduce(c.length, 'sum', lengths=per_field, initial=0.0)
    return route


# ---- connector clearance (fcpp_conn_clear / fcpp_route_transit_clear; the rule: include/fcpp.h) ------------------------------------------
@dataclass
class ConnectorClearance:
    """connector_clearance(): solved connectors against the rings of their fields, one entry per pair"""
    clear: object               # (n) bool: inside and crossings == 0
    crossings: object           # (n) int32: the points where the connector crosses an edge of its field
    inside: object              # (n) int8: even-odd membership of the connector's start point
    first_s: object             # (n) float64: the arc length to the first crossing [m]; +inf without one, NaN for an unsolved pair or a bad field
    length: object              # (n) float64: the connector's length [m]
    field_status: object        # (n_fields) int32: 0, or FCPP_EINVAL (no ring, a ring of fewer than 3 vertices, a non-finite vertex)


def _pair_field(pair_field, n, dev):
    """the field index of every pair, given as one per pair or one for all -> (n) int64, contiguous, on the device"""
    return _one_per(_torch().as_tensor(pair_field, device=dev).to(_torch().int64), n, 'pair_field', 'field index per pair')


def _connector_clearance(frm, to, pf, pair_field, radius, reversing, device):
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    f, t = _poses(frm, dev), _poses(to, dev)
    word, seg, length = _conn_solve(ctx, f, t, radius, reversing)
    n = int(word.numel())
    pair_field = _pair_field(pair_field, n, dev)
    crossings = torch.empty(n, dtype=torch.int32, device=dev)
    inside = torch.empty(n, dtype=torch.int8, device=dev)
    first_s = torch.empty(n, dtype=torch.float64, device=dev)
    status = torch.empty(pf.n, dtype=torch.int32, device=dev)
    L.check(ctx.lib.fcpp_conn_clear(ctx.handle, 1 if reversing else 0, n, _ptr(f[0]), _ptr(f[1]), _ptr(f[2]), float(radius), _ptr(word), _ptr(seg),
                                    _ptr(pair_field), *pf._head(), _ptr(crossings), _ptr(inside), _ptr(first_s), _ptr(status)))
    return ConnectorClearance((inside == 1) & (crossings == 0), crossings, inside, first_s, length, status)


def connector_clearance(from_poses, to_poses, fields, pair_field, radius, reversing=False, device=None):
    """Solve, then test (fcpp_dubins_solve / fcpp_rs_solve + fcpp_conn_clear; the rule: include/fcpp.h): is the shortest Dubins --
    Reeds-Shepp if `reversing` -- connector of every pair from_poses[i] -> to_poses[i] clear of field pair_field[i] of `fields` (what
    polygon_fields takes: rings, even-odd interior)?  The test is exact, piece against edge, not by samples.  pair_field: one index per
    pair (or one for all); -1 means no region: clear.  A margin is no parameter: pass polygon_inset(fields, [margin]).as_fields(0).
    Nothing is re-shaped.  -> ConnectorClearance."""
    return _connector_clearance(from_poses, to_poses, polygon_fields(fields, device), pair_field, radius, reversing, device)


@dataclass
class ClearConnectors:
    """clear_connectors(): per pair the shortest word that stays inside the pair's field, one entry per pair"""
    word: object                # (n) int32: the word driven (-1: unsolved pair)
    seg: object                 # (n, 3) or (n, 5) float64: its segments, as dubins_solve / rs_solve give them
    length: object              # (n) float64: its length [m]
    rank: object                # (n) int32: its position among the pair's candidates by (length, word); 0 the shortest; -1: no word is clear
    crossings: object           # (n) int32: 0 for rank >= 0; for rank -1 the crossings of the shortest word, which is the one returned
    shortest_length: object     # (n) float64: the shortest word's length [m]: what dubins_solve / rs_solve give
    field_status: object        # (n_fields) int32: fcpp_conn_clear's status of every field
    radius: float
    reversing: bool
    _start: object = None       # the prepared start poses
    _device: object = None

    def paths(self, spacing):
        """The words sampled every `spacing` metres by the connectors' own samplers (fcpp_dubins_counts / _sample, fcpp_rs_counts /
        _sample) -> (x, y, heading, kappa, offsets), for reversing=True (x, y, heading, kappa, gear, offsets), as dubins_paths / rs_paths."""
        ctx = get_context(self._device)
        o = _conn_sample_solved(ctx, self._start, self.word, self.seg, self.length, self.radius, spacing, self.reversing)
        if self.reversing:
            return o['x'], o['y'], o['heading'], o['kappa'], o['gear'], o['offsets']
        return o['x'], o['y'], o['heading'], o['kappa'], o['offsets']


def clear_connectors(from_poses, to_poses, fields, pair_field, radius, reversing=False, device=None):
    """Per pair from_poses[i] -> to_poses[i] the SHORTEST Dubins -- Reeds-Shepp if `reversing` -- word that stays inside field
    pair_field[i] of `fields` (fcpp_conn_solve_clear; the rule: include/fcpp.h): the solvers' 6 / 48 candidates in the order (length,
    word), each tested as connector_clearance tests the shortest one, the first clear one kept.  rank says which it was; rank -1: none is
    clear and the shortest word is returned with its crossings.  pair_field: one index per pair (or one for all); -1 means no region.  One
    word per pair -- via points and rides along a headland loop are loop_transits'; a margin is no parameter: pass polygon_inset(fields, [margin]).as_fields(0).  -> ClearConnectors."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    pf = polygon_fields(fields, device)
    f, t = _poses(from_poses, dev), _poses(to_poses, dev)
    n = int(f[0].numel())
    if int(t[0].numel()) != n:
        raise ValueError('from_poses and to_poses must hold the same number of poses')
    pair_field = _pair_field(pair_field, n, dev)
    word = torch.empty(n, dtype=torch.int32, device=dev)
    seg = torch.empty((n, 5 if reversing else 3), dtype=torch.float64, device=dev)
    length = torch.empty(n, dtype=torch.float64, device=dev)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    crossings = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(pf.n, dtype=torch.int32, device=dev)
    shortest = _conn_solve(ctx, f, t, radius, reversing)[2]
    L.check(ctx.lib.fcpp_conn_solve_clear(ctx.handle, 1 if reversing else 0, n, _ptr(f[0]), _ptr(f[1]), _ptr(f[2]), _ptr(t[0]), _ptr(t[1]), _ptr(t[2]),
                                          float(radius), _ptr(pair_field), *pf._head(), _ptr(word), _ptr(seg), _ptr(length), _ptr(rank),
                                          _ptr(crossings), _ptr(status)))
    return ClearConnectors(word, seg, length, rank, crossings, shortest, status, float(radius), bool(reversing), f, device)


@dataclass
class FieldPathClearance:
    """field_path_clearance(): the connector legs of every field's path against its field.  One entry per connector leg that exists,
    ordered by field, then by slot."""
    field: object               # (L) int64: the leg's field
    slot: object                # (L) int32: its leg slot within the field, FieldPaths.leg's numbering: 0 entry, 2 k + 2 behind the k-th swath driven
    clear: object               # (L) bool
    crossings: object           # (L) int32
    first_s: object             # (L) float64: arc length along the leg to its first crossing [m]
    leg_length: object          # (L) float64: the leg's length [m]
    blocked: object             # (n) int32: the legs of the field that are not clear
    length: object              # (n) float64: the field's summed connector length [m]
    field_status: object        # (n) int32: fcpp_conn_clear's status of the field tested against


def _leg_pairs(ss, order, entry, exit):
    """the connector legs of the fields' driving orders, built on the device as field_paths forms them -> (from, to, field, slot), ordered by
    field, then by slot"""
    torch = _torch()
    dev = ss.a.device
    soff_h = np.ascontiguousarray(ss.offsets_host, dtype=np.int64)
    n, m = len(soff_h) - 1, int(soff_h[-1])
    counts = torch.as_tensor(np.diff(soff_h), device=dev)
    fld = _owners(ss.offsets, m)                                                                  # the field of every driven position
    k = torch.arange(m, dtype=torch.int64, device=dev) - ss.offsets[fld]                          # and its rank in the order
    if order is None:
        o = 2 * k + (k & 1)
    else:
        order = order.order if isinstance(order, SwathRoute) else order
        o = torch.as_tensor(order, device=dev).to(torch.int64).reshape(-1)
        if int(o.numel()) != m:
            raise ValueError('order must hold one oriented swath per swath of the SwathSet')
        if m and bool(((o < 0) | (o >= 2 * counts[fld])).any()):
            raise ValueError('order must hold oriented swaths 2 s + d local to their field')
        if m and bool((torch.bincount(ss.offsets[fld] + (o >> 1), minlength=m) != 1).any()):
            raise ValueError('order must hold every swath of a field exactly once (field_paths gives such a field FCPP_EINVAL and no samples)')
    sw, d = ss.offsets[fld] + (o >> 1), (o & 1).to(torch.bool).unsqueeze(1)
    th = ss.angle[fld].unsqueeze(1)
    h = torch.where(d, th + np.pi, th)
    ent = torch.cat([torch.where(d, ss.b[sw], ss.a[sw]), h], dim=1)                               # where the oriented swath is entered / left
    ext = torch.cat([torch.where(d, ss.a[sw], ss.b[sw]), h], dim=1)
    inner = k + 1 < counts[fld]
    frm, to, lf, slot = [ext[inner]], [ent[1:][inner[:-1]]], [fld[inner]], [2 * k[inner] + 2]
    has = torch.nonzero(counts > 0).reshape(-1)
    first, last = ss.offsets[has], ss.offsets[has + 1] - 1
    if entry is not None:
        p = torch.stack(_pose_columns(entry, n, dev), dim=1)
        frm.append(p[has]); to.append(ent[first]); lf.append(has); slot.append(torch.zeros_like(has))
    if exit is not None:
        p = torch.stack(_pose_columns(exit, n, dev), dim=1)
        frm.append(ext[last]); to.append(p[has]); lf.append(has); slot.append(2 * counts[has])
    frm, to, lf, slot = torch.cat(frm), torch.cat(to), torch.cat(lf), torch.cat(slot)
    by_slot = torch.argsort(2 * ss.offsets[lf] + lf + slot)                                       # a field's first slot is 2 soff + i
    return frm[by_slot].contiguous(), to[by_slot].contiguous(), lf[by_slot], slot[by_slot]


def _legs_clearance(ss, pf, R, reversing, order, entry, exit, device):
    """the connector legs of the fields' driving orders (_leg_pairs), solved at R and tested"""
    torch = _torch()
    dev = ss.a.device
    n = len(ss.offsets_host) - 1
    frm, to, lf, slot = _leg_pairs(ss, order, entry, exit)
    c = _connector_clearance(frm, to, pf, lf, R, reversing, device)
    blocked = torch.zeros(n, dtype=torch.int32, device=dev)
    blocked.index_add_(0, lf, (~c.clear).to(torch.int32))
    # a field's lengths summed in slot order, one segment per field (an atomic float sum has no fixed order)
    length = torch.segment_reduce(c.length, 'sum', lengths=torch.bincount(lf, minlength=n), initial=0.0)
    return FieldPathClearance(lf, slot.to(torch.int32), c.clear, c.crossings, c.first_s, c.length, blocked, length, c.field_status)


def field_path_clearance(swathset, fields, radius, spacing, reversing=False, order=None, entry=None, exit=None, device=None):
    """The connector legs field_paths drives -- same order, entry / exit, and _chord_radius(radius, spacing) -- tested against `fields`
    (one per field of the SwathSet, as polygon_fields takes them): the legs' poses are formed on the device, solved and passed to
    fcpp_conn_clear.  -> FieldPathClearance: per connector leg clear / crossings / first_s under FieldPaths.leg's slot numbering, and the
    blocked legs per field (what route_swaths(clear_of=...) reports as SwathRoute.blocked / .clearance for the same arguments).  The swath
    legs are not tested: they lie in the work area they were cut from.  An order that is no permutation of a field's swaths raises
    ValueError here (field_paths gives that field FCPP_EINVAL and no samples)."""
    n = len(swathset.offsets_host) - 1
    return _legs_clearance(swathset, _clear_fields(fields, n, device), _chord_radius(radius, spacing), reversing, order, entry, exit, device)


# ---- field paths (fcpp_field_path_counts / _fill; the rule: include/fcpp.h) -------------------------------------------------------------
@dataclass
class PathSet:
    """Sampled paths in the CSR form curvature(), speed_plan(), validate() and trajectory() take (offsets=): path p owns the samples
    offsets[p] .. offsets[p + 1].  What every path-set result of the polygon chain begins with; the methods say what the consumers
    (polygon_coverage, mission_paths, loop_transits) need to know of a set, and the kinds of set override them."""
    offsets: object             # (n + 1) int64, device; offsets_host: the numpy copy
    offsets_host: object
    x: object                   # (total) float64
    y: object
    heading: object             # (total) float64, in (-pi, pi]: the vehicle's heading
    kappa: object               # (total) float64: signed curvature
    part: object                # (total) int8: the FCPP_PART_* of the sample
    gear: object                # (total) int8: +1, -1 on the reverse runs of a Reeds-Shepp connector

    closed = False              # whether every path is a loop (its last sample joins its first)

    def path(self, i):
        """(x, y, heading, part) of path i: swath_route's tuple"""
        sl = slice(int(self.offsets_host[i]), int(self.offsets_host[i + 1]))
        return self.x[sl], self.y[sl], self.heading[sl], self.part[sl]

    def _paths(self, dtype=None):
        return _torch().arange(int(self.offsets.numel()) - 1, dtype=dtype or _torch().int64, device=self.x.device)

    def path_field(self):
        """(n) int64: the field of every path; path i is field i's"""
        return self._paths()

    def drive_order(self, innermost_first=False):
        """(n) int64: the order in which a mission drives the set's paths; as stored"""
        return self._paths()

    def work(self):
        """(total) bool: the samples that work (cover); the straight work parts, 0 and 4"""
        return (self.part == 0) | (self.part == 4)

    def pass_id(self):
        """(total) int32: the id of the pass a sample belongs to (two different ids over one cell overlap); the path's index"""
        return _owners(self.offsets, int(self.x.numel()), _torch().int32)


@dataclass
class FieldPaths(PathSet):
    """field_paths(): one sampled path per field of a SwathSet: a PathSet whose path i is field i's.  kappa is 0 on a swath; part: 0 swath,
    1 connector between swaths, 2 entry connector, 3 exit connector."""
    leg: object                 # (total) int32: the leg slot within the field: 0 entry, 2 k + 1 the k-th swath driven, 2 k + 2 the connector behind it
    work_length: object         # (n) float64: the swath lengths in driving order [m]
    transit_length: object      # (n) float64: the connector lengths, entry and exit included [m]: the route's cost
    status: object              # (n) int32: 0, or FCPP_EINVAL (an order that is no permutation, a non-finite length or pose): no samples
    leg_offsets: object         # (2 m_total + n + 1) int64: the first sample of every leg slot; field i's first slot is 2 swath_offsets[i] + i
    # field_paths(clear_of=...) only (None otherwise); per leg slot like leg_offsets, the rule: include/fcpp.h, "clear field paths"
    leg_rank: object = None     # int32: the driven word's place among the pair's candidates; -1: no candidate is clear, the shortest is driven
    leg_crossings: object = None    # int32: the driven word's boundary crossings (0 unless rank is -1)
    leg_word: object = None     # int32: the driven connector's word, -1 on a slot that is no connector
    leg_seg: object = None      # (slots, 5) float64: its segments (a swath's end point and length in [0 .. 2])
    leg_total: object = None    # float64: its length
    blocked: object = None      # (n) int32: the field's connector legs of rank -1
    reshaped: object = None     # (n) int32: the field's connector legs of rank > 0
    region_status: object = None    # (n) int32: 0, or FCPP_EINVAL for a region field with no ring, a ring of fewer than 3 vertices, a non-finite vertex
    # field_paths(clear_of=..., loops=...) only (None otherwise): the rank -1 legs that ride a headland loop round the obstacle.  Plain
    # attributes set on the result, not constructor arguments: the members above are the entries' outputs in their order
    detoured = None             # (n) int32: the field's connector legs whose samples are a loop transit's; `blocked` counts the rest
    leg_transit = None          # (slots) int64: the slot's index into `transits`, -1 where the slot's own record is driven
    transits = None             # LoopTransits of the rank -1 legs, ordered by field, then by slot

    field = PathSet.path        # (x, y, heading, part) of field i

    def work(self):
        """the swaths"""
        return self.part == 0

    def pass_id(self):
        """the leg"""
        return self.leg


def _pose_columns(pose, n, dev):
    """one pose (x, y, heading) per field -> three contiguous device columns (or three None)"""
    if pose is None:
        return None, None, None
    p = _dev_f64(pose, dev).reshape(-1, 3)
    if p.shape[0] != n:
        raise ValueError('entry / exit must hold one pose (x, y, heading) per field')
    p = p.t().contiguous()
    return p[0], p[1], p[2]


def _leg_paths(ctx, counts, fill, args, n_groups, n_slots, n_totals, dev):
    """What field_paths and headland_paths share: the counts entry, the total read from its host offsets, the seven sample columns, the fill
    entry -> (offsets, offsets_host, x, y, heading, kappa, part, gear, leg, *totals, status, leg_offsets).  args: the entries' common
    arguments behind the handle; n_totals: the per-group float64 totals the counts entry writes."""
    torch = _torch()
    leg_off = torch.empty(n_slots + 1, dtype=torch.int64, device=dev)
    totals = [torch.empty(n_groups, dtype=torch.float64, device=dev) for _ in range(n_totals)]
    status = torch.empty(n_groups, dtype=torch.int32, device=dev)
    ctx.bind_stream()
    samples = _counts_fill(n_groups, dev, lambda off, off_h: counts(ctx.handle, *args, off, off_h, _ptr(leg_off), *[_ptr(t) for t in totals], _ptr(status)),
                           lambda off, off_h, total, *cols: fill(ctx.handle, *args, _ptr(leg_off), total, *cols), _sample_columns(torch.int32))
    return (*samples, *totals, status, leg_off)


def field_paths(swathset, radius, spacing, reversing=False, order=None, entry=None, exit=None, device=None, clear_of=None, loops=None):
    """The path of EVERY field of a SwathSet in one pass on the device (fcpp_field_path_counts + fcpp_field_path_fill) -> FieldPaths.
    What swath_route gives for one field, for the whole batch and without a host loop: each swath sampled every `spacing` metres (its last
    sample is its end), consecutive swaths joined by the shortest Dubins path -- Reeds-Shepp if `reversing` -- planned at
    _chord_radius(radius, spacing) exactly as swath_route plans it, junction samples doubled.  order: None (the stored boustrophedon), a
    SwathRoute of the same SwathSet (route_swaths: pass it the same `spacing`) or an int array of m_total oriented swaths, each field's
    local to it.  entry / exit: one pose (x, y, heading) per field, as route_swaths takes them: the connectors it priced are driven (part 2
    and 3).  A field whose order is no permutation of its swaths, or with a non-finite length or pose, has status FCPP_EINVAL and no samples;
    the others are unaffected.  Connectors know no boundary (validate() flags what leaves the field) unless `clear_of` is given to
    route_swaths; field_path_clearance tests the connectors driven here.
    clear_of (a PolygonFields or anything polygon_fields takes, one region per field of the SwathSet): every connector drives the shortest
    word that stays off its region's rings, as clear_connectors chooses it (fcpp_field_path_counts_clear + fcpp_field_path_fill_clear);
    where no word is clear the shortest is still driven.  FieldPaths then holds leg_rank, leg_crossings, leg_word, leg_seg, leg_total
    per leg slot and blocked, reshaped, region_status per field; connector_clearance on the legs' start poses, leg_word and leg_seg
    agrees with leg_rank.  Without clear_of nothing changes, down to the entries called.
    loops (with clear_of; a HeadlandPaths or a sequence of them, e.g. both directions): every rank -1 leg for which loop_transits finds a
    transit -- a clear connector onto a headland loop, a ride along it, a clear connector off it -- has its samples replaced by the
    transit's (part 1 on its connectors, FCPP_PART_LOOP_RIDE on the ride; `leg` stays the slot).  offsets, leg_offsets and transit_length
    follow; blocked counts the legs that are still driven through the region, detoured those that ride; leg_transit and transits say
    which.  The per-slot records (leg_word, leg_seg, leg_total, leg_rank) stay those of the word that was not driven.  The ride itself is
    not tested against the region.  Without loops nothing changes, down to the entries called."""
    if loops is not None and clear_of is None:
        raise ValueError('loops needs clear_of: the region the transits have to stay clear of')
    ctx = get_context(device)
    torch = _torch()
    ss = swathset
    dev = ss.a.device
    soff_h = np.ascontiguousarray(ss.offsets_host, dtype=np.int64)
    n, m = len(soff_h) - 1, int(soff_h[-1])
    if order is not None:
        order = order.order if isinstance(order, SwathRoute) else order
        order = torch.as_tensor(order, device=dev).to(torch.int32).reshape(-1).contiguous()
        if int(order.numel()) != m:
            raise ValueError('order must hold one oriented swath per swath of the SwathSet')
    ax, ay, bx, by = (t[:, k].contiguous() for t in (ss.a, ss.b) for k in (0, 1))
    ent, ext = _pose_columns(entry, n, dev), _pose_columns(exit, n, dev)
    args = (n, _ptr(ss.offsets), _host_ptr(soff_h), m, _ptr(ax), _ptr(ay), _ptr(bx), _ptr(by), _ptr(ss.length), _ptr(ss.angle), _ptr(order),
            _chord_radius(radius, spacing), 1 if reversing else 0, float(spacing), *[_ptr(t) for t in ent], *[_ptr(t) for t in ext])
    if clear_of is None:
        return FieldPaths(*_leg_paths(ctx, ctx.lib.fcpp_field_path_counts, ctx.lib.fcpp_field_path_fill, args, n, 2 * m + n, 2, dev))
    pf = _clear_fields(clear_of, n, device)          # (holds the region's tensors until the entries have returned)
    region = pf._head()[1:]
    n_slots = 2 * m + n
    slot_i32 = lambda: torch.empty(n_slots, dtype=torch.int32, device=dev)
    field_i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)
    extra = (slot_i32(), slot_i32(), slot_i32(), torch.empty((n_slots, 5), dtype=torch.float64, device=dev),
             torch.empty(n_slots, dtype=torch.float64, device=dev), field_i32(), field_i32(), field_i32())

    def counts(handle, *a):
        return ctx.lib.fcpp_field_path_counts_clear(handle, *a, *[_ptr(t) for t in extra])

    fp = FieldPaths(*_leg_paths(ctx, counts, ctx.lib.fcpp_field_path_fill_clear, args + tuple(region), n, n_slots, 2, dev), *extra)
    if loops is None:
        return fp
    return _detour_field_paths(fp, ss, pf, loops, _chord_radius(radius, spacing), spacing, reversing, order, entry, exit, device)


# ---- headland paths (fcpp_headland_path_counts / _fill; the rule: include/fcpp.h) -------------------------------------------------------
@dataclass
class HeadlandPaths(PathSet):
    """headland_paths(): one sampled, closed path per ring of an InsetSet: a PathSet whose path r is ring r.  kappa is 0 on a straight
    element, -/+ 1 / d on a followed arc; part: 0 straight element, 1 connector, 4 followed arc."""
    leg: object                 # (total) int32: the leg slot within the ring: 2 k the element driven vertex k starts, 2 k + 1 the joint behind it
    work_length: object         # (n_rings) float64: the straight elements and followed arcs [m]
    transit_length: object      # (n_rings) float64: the connectors [m]
    skipped_length: object      # (n_rings) float64: the arcs too tight to follow, bridged by a connector [m]
    status: object              # (n_rings) int32: 0, FCPP_EINVAL or FCPP_EUNSUPPORTED (no drivable element): no samples
    leg_offsets: object         # (2 n_verts + 1) int64: the first sample of every leg slot; ring r's first slot is 2 ring_offsets[r]
    ring_pair: object           # (n_rings, 2) int64, device: the (field, pass) index of every ring
    spacing: object = None      # the sample spacing the loops were driven at [m] (loop_transits turns station_step into a stride by it)

    closed = True
    ring = PathSet.path         # (x, y, heading, part) of ring r

    def path_field(self):
        """the ring's field"""
        return self.ring_pair[:, 0]

    def drive_order(self, innermost_first=False):
        """as stored, or (stable) the innermost pass first"""
        return _torch().argsort(-self.ring_pair[:, 1], stable=True) if innermost_first else self._paths()

    def pass_id(self):
        """-1 - ring: negative, distinct from a field path's legs (work: the base's, the straight elements and the followed arcs)"""
        return -1 - _owners(self.offsets, int(self.x.numel()), _torch().int32)


def _headland_paths(ctx, ring_offsets, x, y, src, ring_dist, R, mode, spacing, direction, smooth_tol, ring_offsets_host=None):
    """the two C entries on device tensors; R as it is (no chord radius) -> the HeadlandPaths fields but ring_pair"""
    dev = x.device
    nr, nv = int(ring_offsets.numel()) - 1, int(x.numel())
    roff_h = None if ring_offsets_host is None else np.ascontiguousarray(ring_offsets_host, dtype=np.int64)
    args = (nr, _ptr(ring_offsets), _host_ptr(roff_h), nv, _ptr(x), _ptr(y), _ptr(src), _ptr(ring_dist), float(R), int(mode), float(spacing),
            int(direction), float(smooth_tol))
    return _leg_paths(ctx, ctx.lib.fcpp_headland_path_counts, ctx.lib.fcpp_headland_path_fill, args, nr, 2 * nv, 3, dev)


def headland_paths(inset, radius, spacing, reversing=False, direction=1, smooth_tol=1e-6, device=None):
    """EVERY ring of an InsetSet (headland()'s pass centre lines: all fields, all passes) as one sampled, closed, drivable path each, in one
    pass on the device (fcpp_headland_path_counts + fcpp_headland_path_fill) -> HeadlandPaths.  The straight pieces are driven to their
    very ends and sampled every `spacing` metres; the arcs around reflex vertices are followed where the pass's distance d is at least the
    planning radius _chord_radius(radius, spacing) (as field_paths plans) and bridged where it is not (skipped_length); every joint whose
    heading jumps by more than smooth_tol [rad] is closed by the shortest Dubins path -- Reeds-Shepp if `reversing` -- which at a sharp
    corner is the bulb turn or the three-point turn.  direction +1 drives a ring as stored (kept area on the left), -1 the other way round;
    both start at the ring's first vertex.  A ring with a non-finite vertex has status FCPP_EINVAL, one without a drivable element
    FCPP_EUNSUPPORTED; such rings have no samples and the others are unaffected.  Connectors know no boundary (validate() flags what leaves
    the field)."""
    ctx = get_context(device)
    torch = _torch()
    dev = inset.x.device
    nr = int(inset.ring_offsets.numel()) - 1
    pair = _owners(inset.pair_ring_offsets, nr)
    D = max(inset.D, 1)
    ring_pair = torch.stack([pair // D, pair % D], dim=1)
    ring_dist = inset.distances[ring_pair[:, 1]].contiguous() if nr else torch.empty(0, dtype=torch.float64, device=dev)
    out = _headland_paths(ctx, inset.ring_offsets, inset.x, inset.y, inset.src, ring_dist, _chord_radius(radius, spacing), 1 if reversing else 0,
                          spacing, direction, smooth_tol)
    return HeadlandPaths(*out, ring_pair, float(spacing))


# ---- loop transits (fcpp_loop_transit_solve / _counts / _fill; the rule: include/fcpp.h) ------------------------------------------------
@dataclass
class TransitPaths(PathSet):
    """LoopTransits.paths(): one sampled path per pair -- a pair that is not found has no samples.  part: 1 on the two connectors,
    FCPP_PART_LOOP_RIDE (5) on the ride."""


@dataclass
class LoopTransits:
    """loop_transits(): per pair the cheapest "clear connector onto a loop, ride, clear connector off it", one entry per pair"""
    found: object               # (n) int32
    loop: object                # (n) int64: the loop ridden, an index into the loop set as loop_transits arranged it (loops sorted by field); -1
    st_i: object                # (n) int64: the stations where the ride starts and ends, sample indices into that loop set; -1
    st_j: object
    in_word: object             # (n) int32, (n, 3 / 5), (n), (n) int32: the connector onto the loop, as clear_connectors gives it
    in_seg: object
    in_length: object
    in_rank: object
    out_word: object            # the connector off the loop
    out_seg: object
    out_length: object
    out_rank: object
    ride: object                # (n) float64: the arc length ridden [m]
    total: object               # (n) float64: in + ride + out [m]; +inf where no transit is found
    status: object              # (n) int32: 0, FCPP_EINVAL (a non-finite pose, a bad region or loop field), FCPP_EUNSUPPORTED (too many stations)
    radius: float
    reversing: bool
    stride: int
    loop_set: object = None     # dict of the arranged loop set's device tensors: offsets, x, y, heading, kappa, s, part, gear, field_loops
    _start: object = None
    _device: object = None

    def paths(self, spacing):
        """The transits sampled (fcpp_loop_transit_counts + fcpp_loop_transit_fill): the connectors every `spacing` metres by the
        connectors' own samplers, the ride the loop's own samples -> TransitPaths."""
        ctx = get_context(self._device)
        ls, f = self.loop_set, self._start
        n = int(self.found.numel())
        mode = 1 if self.reversing else 0
        rec = [_ptr(t) for t in (self.found, self.loop, self.st_i, self.st_j, self.in_word, self.in_seg, self.out_word, self.out_seg)]
        lhead = (int(ls['offsets'].numel()) - 1, _ptr(ls['offsets']), _host_ptr(ls['offsets_host']), int(ls['x'].numel()))
        ctx.bind_stream()
        return TransitPaths(*_counts_fill(
            n, self.found.device, lambda *off: ctx.lib.fcpp_loop_transit_counts(ctx.handle, mode, n, *rec, *lhead, float(spacing), *off),
            lambda *out: ctx.lib.fcpp_loop_transit_fill(ctx.handle, mode, n, _ptr(f[0]), _ptr(f[1]), _ptr(f[2]), float(self.radius), *rec, *lhead,
                                                        _ptr(ls['x']), _ptr(ls['y']), _ptr(ls['heading']), _ptr(ls['kappa']), _ptr(ls['gear']),
                                                        float(spacing), *out), _sample_columns()))


def _loop_set(loops, n_fields, dev, device):
    """HeadlandPaths (one or several, e.g. both directions) -> the loop set of the transit entries: the loops sorted by field (stable: a
    field's loops in the order given), their samples gathered, s from trajectory(), field_loops from ring_pair -> (dict, spacing)"""
    torch = _torch()
    loops = [loops] if isinstance(loops, PathSet) else list(loops)
    names = ('x', 'y', 'heading', 'kappa', 's', 'part', 'gear')
    cols, spacing = [], None
    for hp in loops:
        total = int(hp.x.numel())
        s = trajectory(hp.x, hp.y, torch.ones(total, dtype=torch.float64, device=dev), offsets=hp.offsets, device=device)[0] if total else hp.x
        cols.append((hp.x, hp.y, hp.heading, hp.kappa, s, hp.part, hp.gear))
        spacing = hp.spacing if spacing is None else spacing
    _, _, joined, _, cols = _join_csr([hp.offsets for hp in loops], [None] * len(loops), cols, (torch.float64,) * 5 + (torch.int8,) * 2, dev)
    i64 = lambda ts: torch.cat(ts) if ts else torch.zeros(0, dtype=torch.int64, device=dev)
    order, fl = _group_by(i64([hp.path_field().to(dev) for hp in loops]), n_fields)
    start, lens = joined[:-1][order], (joined[1:] - joined[:-1])[order]
    off = torch.zeros(int(lens.numel()) + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(lens, 0)
    off_h = off.cpu().numpy()
    total = int(off_h[-1])
    idx = torch.repeat_interleave(start - off[:-1], lens, output_size=total) + torch.arange(total, dtype=torch.int64, device=dev)
    ls = {k: c[idx].contiguous() for k, c in zip(names, cols)}
    ls.update(offsets=off, offsets_host=off_h, field_loops=fl, field_loops_host=fl.cpu().numpy())
    if spacing is None:          # (loops that do not say: the mean step of their samples)
        steps = total - int(lens.numel())
        last = off[1:][lens > 0] - 1
        spacing = float(ls['s'][last].sum()) / steps if steps > 0 else 1.0
    return ls, spacing


def _loop_transits(ctx, f, t, pf, pair_field, ls, radius, reversing, stride, device):
    torch = _torch()
    dev = f[0].device
    n = int(f[0].numel())
    ns = 5 if reversing else 3
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)
    i64 = lambda: torch.empty(n, dtype=torch.int64, device=dev)
    f64 = lambda *shape: torch.empty((n,) + shape, dtype=torch.float64, device=dev)
    out = (i32(), i64(), i64(), i64(), i32(), f64(ns), f64(), i32(), i32(), f64(ns), f64(), i32(), f64(), f64(), i32())
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_loop_transit_solve(ctx.handle, 1 if reversing else 0, n, _ptr(f[0]), _ptr(f[1]), _ptr(f[2]), _ptr(t[0]), _ptr(t[1]), _ptr(t[2]),
                                            float(radius), _ptr(pair_field), *pf._head(), int(ls['offsets'].numel()) - 1, _ptr(ls['offsets']),
                                            _host_ptr(ls['offsets_host']), int(ls['x'].numel()), _ptr(ls['x']), _ptr(ls['y']), _ptr(ls['heading']),
                                            _ptr(ls['s']), _ptr(ls['part']), _ptr(ls['gear']), _ptr(ls['field_loops']), _host_ptr(ls['field_loops_host']),
                                            int(stride), *[_ptr(o) for o in out]))
    return LoopTransits(*out, float(radius), bool(reversing), int(stride), ls, f, device)


def loop_transits(from_poses, to_poses, fields, pair_field, loops, radius, reversing=False, station_step=None, device=None):
    """Per pair from_poses[i] -> to_poses[i] the cheapest LOOP TRANSIT (fcpp_loop_transit_solve; the rule: include/fcpp.h): the shortest clear
    Dubins -- Reeds-Shepp if `reversing` -- connector (as clear_connectors chooses it, against field pair_field[i] of `fields`) onto a
    station of one of the field's headland loops, a ride forwards along that loop, and the shortest clear connector off it, over all loops
    of the field and all pairs of stations.  loops: a HeadlandPaths or a sequence of them (pass direction=+1 and direction=-1 to offer both
    ways round); a loop serves the field its ring belongs to (ring_pair).  Stations: every max(1, round(station_step / spacing)) -th
    sample of a loop that lies on a straight element or a followed arc; station_step defaults to `radius`.  At most
    FCPP_TRANSIT_MAX_STATIONS stations per field (status FCPP_EUNSUPPORTED beyond: raise station_step).  pair_field: one index per pair (or
    one for all), 0 .. n_fields - 1.  The ride is not tested against the region: a headland pass lies inside its field by construction,
    its corner connectors may not (validate() flags that).  -> LoopTransits; .paths(spacing) samples them."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    pf = polygon_fields(fields, device)
    f, t = _poses(from_poses, dev), _poses(to_poses, dev)
    n = int(f[0].numel())
    if int(t[0].numel()) != n:
        raise ValueError('from_poses and to_poses must hold the same number of poses')
    pair_field = _pair_field(pair_field, n, dev)
    ls, spacing = _loop_set(loops, pf.n, dev, device)
    step = float(radius) if station_step is None else float(station_step)
    if not step > 0.0:
        raise ValueError('station_step must be positive')
    return _loop_transits(ctx, f, t, pf, pair_field, ls, radius, reversing, max(1, int(round(step / spacing))), device)


def _detour_field_paths(fp, ss, pf, loops, R, spacing, reversing, order, entry, exit, device):
    """field_paths(loops=...): the rank -1 legs of a clear field path through loop_transits at the planning radius R; the found ones'
    samples spliced in by one gather on the device"""
    ctx = get_context(device)
    torch = _torch()
    dev = fp.x.device
    soff_h = np.ascontiguousarray(ss.offsets_host, dtype=np.int64)
    n, m = len(soff_h) - 1, int(soff_h[-1])
    n_slots = 2 * m + n
    frm, to, lf, slot = _leg_pairs(ss, order, entry, exit)
    g = 2 * ss.offsets[lf] + lf + slot                                   # the legs' global slots
    ok = fp.status[lf] == 0 if int(lf.numel()) else torch.zeros(0, dtype=torch.bool, device=dev)
    pick = torch.nonzero(ok & (fp.leg_rank[g] < 0) & (fp.leg_word[g] >= 0)).reshape(-1)
    g, lf, slot = g[pick], lf[pick].contiguous(), slot[pick]
    f = tuple(frm[pick][:, k].contiguous() for k in range(3))
    t = tuple(to[pick][:, k].contiguous() for k in range(3))
    ls, loop_spacing = _loop_set(loops, n, dev, device)
    lt = _loop_transits(ctx, f, t, pf, lf, ls, R, reversing, max(1, int(round(R / loop_spacing))), device)
    tp = lt.paths(spacing)
    leg_transit = torch.full((n_slots,), -1, dtype=torch.int64, device=dev)
    hit = lt.found == 1
    leg_transit[g[hit]] = torch.nonzero(hit).reshape(-1)
    detoured = torch.zeros(n, dtype=torch.int32, device=dev)
    detoured.index_add_(0, lf[hit], torch.ones(int(hit.sum()), dtype=torch.int32, device=dev))
    # the gather: per slot where its samples start in [the plain path's samples; the transits' samples] and how many they are
    old_off, plain_total = fp.leg_offsets, int(fp.x.numel())
    cnt, src = old_off[1:] - old_off[:-1], old_off[:-1].clone()
    det = leg_transit >= 0
    tr = leg_transit[det]
    cnt[det] = tp.offsets[tr + 1] - tp.offsets[tr]
    src[det] = plain_total + tp.offsets[tr]
    leg_off = torch.zeros(n_slots + 1, dtype=torch.int64, device=dev)
    leg_off[1:] = torch.cumsum(cnt, 0)
    first = 2 * ss.offsets + torch.arange(n + 1, dtype=torch.int64, device=dev)
    first[n] = n_slots
    off = leg_off[first].contiguous()
    off_h = off.cpu().numpy()
    total = int(off_h[-1])
    idx = torch.repeat_interleave(src - leg_off[:-1], cnt, output_size=total) + torch.arange(total, dtype=torch.int64, device=dev)
    t_cnt = tp.offsets[1:] - tp.offsets[:-1]
    t_leg = torch.repeat_interleave(slot.to(torch.int32), t_cnt, output_size=int(tp.x.numel()))
    both = lambda a, b: torch.cat([a, b])[idx].contiguous()
    # a detoured field's transit length: its connector slots' lengths in slot order, a detoured slot's the transit's total
    leg_len = fp.leg_total.clone()
    leg_len[g[hit]] = lt.total[hit]
    slots_of = first[1:] - first[:-1]
    fld_of = _owners(first, n_slots)
    even = (torch.arange(n_slots, dtype=torch.int64, device=dev) - first[fld_of]) % 2 == 0
    per_field = (slots_of + 1) // 2
    summed = torch.segment_reduce(leg_len[even], 'sum', lengths=per_field, initial=0.0)
    transit = torch.where(detoured > 0, summed, fp.transit_length)
    out = FieldPaths(off, off_h, both(fp.x, tp.x), both(fp.y, tp.y), both(fp.heading, tp.heading), both(fp.kappa, tp.kappa), both(fp.part, tp.part),
                     both(fp.gear, tp.gear), both(fp.leg, t_leg), fp.work_length, transit, fp.status, leg_off, fp.leg_rank, fp.leg_crossings,
                     fp.leg_word, fp.leg_seg, fp.leg_total, fp.blocked - detoured, fp.reshaped, fp.region_status)
    out.detoured, out.leg_transit, out.transits = detoured, leg_transit, lt
    return out


# ---- mission paths (fcpp_mission_solve / _counts / _fill; the rule: include/fcpp.h) ------------------------------------------------------
@dataclass
class MissionPaths(PathSet):
    """mission_paths(): ONE sampled path per field -- its items joined in driving order: a PathSet whose path i is field i's.  part: the
    source sample's part, FCPP_PART_JOIN (6) on a joint."""
    slot: object               # (total) int32: the slot within the field: 2 j the joint into kept item j, 2 j + 1 the item, the last the exit joint
    src: object                 # (total) int64: the source sample's index into the concatenated item sets, -1 on a joint
    src_set: object             # (total) int32: the position in `items` of the set the sample was copied from, -1 on a joint
    status: object              # (n) int32: 0, FCPP_EINVAL (a chosen pose that is not finite), FCPP_EUNSUPPORTED (a loop of more than 1024 stations): no samples
    transit_length: object      # (n) float64: the joints' lengths in driving order [m]
    skipped: object             # (n) int32: the items without a sample or, closed, without a station: they drive nothing
    item_offsets: object        # (n + 1) int64: field i's items are item_offsets[i] .. item_offsets[i + 1], in driving order
    item_path: object           # (items) int64: the path driven, an index into the concatenated item sets
    item_closed: object         # (items) int32
    item_set: object            # (items) int32: the position in `items` of the item's set
    item_station: object        # (items) int64: the sample a loop is entered and left at (an index like src); -1 for an open or a skipped item
    slot_offsets: object        # (2 items + n + 1) int64: the first sample of every slot; field i's first slot is 2 item_offsets[i] + i
    slot_item: object           # (slots) int64: the item of an item slot, else -1
    slot_word: object           # (slots) int32: a joint's word, else -1
    slot_seg: object            # (slots, 5) float64: its segments
    slot_total: object          # (slots) float64: its length
    radius: float               # the planning radius the joints were solved at
    reversing: bool
    stride: int
    set_starts: object = None   # (sets + 1) numpy int64: where every set's samples start in the concatenation
    blocked: object = None      # (n) int32 with clear_of: the field's joints for which no word is clear of its region (they are driven as they are)

    field = PathSet.path        # (x, y, heading, part) of field i

    def cover_set(self, pass_ids=None, work=None):
        """The tuple (offsets, x, y, path_field, work, pass) polygon_coverage takes, gathered through src.  pass_ids / work: one entry per
        set of `items`, each a tensor per source sample of that set or None -- the set's own work() and pass_id(), what polygon_coverage uses
        for it (a FieldPaths: the swaths, the leg; a HeadlandPaths: straight elements and followed arcs, -1 - ring); a tuple-form set needs
        both given.  Joints do not work."""
        torch = _torch()
        dev = self.x.device
        n_sets = len(self._sets)
        pass_ids = [None] * n_sets if pass_ids is None else list(pass_ids)
        work = [None] * n_sets if work is None else list(work)
        if len(pass_ids) != n_sets or len(work) != n_sets:
            raise ValueError('pass_ids and work take one entry (or None) per item set')
        ws, ps = [], []
        for k, st in enumerate(self._sets):
            total = int(self.set_starts[k + 1] - self.set_starts[k])
            w, p = work[k], pass_ids[k]
            if (w is None or p is None) and not isinstance(st, PathSet):
                raise ValueError('a tuple-form item set needs its pass ids and work flags given')
            w, p = (st.work() if w is None else w), (st.pass_id() if p is None else p)
            w =(torch.as_tensor(w, device=dev).reshape(-1) != 0).to(torch.uint8)
            p = torch.as_tensor(p, device=dev).to(torch.int32).reshape(-1)
            if int(w.numel()) != total or int(p.numel()) != total:
                raise ValueError('pass_ids and work hold one value per sample of their set')
            ws.append(w); ps.append(p)
        copied = self.src >= 0
        at = self.src.clamp(min=0)
        cat = lambda ts, dt: torch.cat(ts + [torch.zeros(1, dtype=dt, device=dev)])          # (one spare element: a set list without a sample)
        w = torch.where(copied, cat(ws, torch.uint8)[at], torch.zeros((), dtype=torch.uint8, device=dev))
        pas = torch.where(copied, cat(ps, torch.int32)[at], torch.zeros((), dtype=torch.int32, device=dev))
        return (self.offsets, self.x, self.y, self.path_field(), w, pas)

    _sets = ()


def _mission_set(st, dev, innermost_first):
    """mission_paths' normaliser: a PathSet, or the tuple (offsets, x, y, heading, kappa, part, gear, field, closed) -> (PathSet, the field
    of every path int64, closed, the paths' order within the set)"""
    torch = _torch()
    if isinstance(st, PathSet):
        return st, st.path_field().to(dev), st.closed, st.drive_order(innermost_first).to(dev)
    offsets, x, y, heading, kappa, part, gear, field, closed = st
    x = _dev_f64(x, dev).reshape(-1)
    total = int(x.numel())
    off, off_h = _offsets(offsets, total, dev)
    npth = int(off.numel()) - 1
    field = torch.as_tensor(field, device=dev).to(torch.int64).reshape(-1)
    if field.numel() == 1 and npth != 1:
        field = field.expand(npth)
    i8 = lambda a: torch.as_tensor(a, device=dev).to(torch.int8).reshape(-1).contiguous()
    ps = PathSet(off, off_h, x, _dev_f64(y, dev).reshape(-1), _dev_f64(heading, dev).reshape(-1), _dev_f64(kappa, dev).reshape(-1), i8(part), i8(gear))
    if any(int(c.numel()) != total for c in (ps.y, ps.heading, ps.kappa, ps.part, ps.gear)) or int(field.numel()) != npth:
        raise ValueError('an item set needs six columns of one length and one field per path')
    return ps, field.contiguous(), bool(closed), ps.drive_order()


@dataclass
class _MissionTable:
    """_mission_table(): the item sets of a mission as the mission entries take them"""
    n: int                      # fields
    first: object               # (sets + 1) numpy int64: where every set's paths start among the joined paths
    starts: object              # (sets + 1) numpy int64: and its samples among the joined samples
    paths: object               # PathSet: the sets joined, offsets_host always there
    ioff: object                # (n + 1) int64: field i's items are ioff[i] .. ioff[i + 1], in driving order; ioff_h: the numpy copy
    ioff_h: object
    ipath: object               # (items) int64: the joined path an item drives; ipath_h: the numpy copy
    ipath_h: object
    iset: object                # (items) int32: the position in `items` of the item's set
    iclosed: object             # (items) int32: whether it is a loop
    longest: int                # the samples of the longest loop, 0 without one


def _mission_table(items, dev, innermost_first=False, n_fields=None, entry=None, exit=None):
    """the item sets joined into one path set and the fields' item table, as fcpp_mission_solve takes them -> _MissionTable"""
    n = n_fields
    torch = _torch()
    sets = [_mission_set(st, dev, innermost_first) for st in items]
    if n is None:
        n = max([int(f.max()) + 1 for _, f, _, _ in sets if int(f.numel())] + [0])
        for p in (entry, exit):
            n = n if p is None else max(n, int(torch.as_tensor(p).reshape(-1, 3).shape[0]))
    first, starts, poff, poff_h, cols = _join_csr([ps.offsets for ps, *_ in sets], [ps.offsets_host for ps, *_ in sets],
                                                  [(ps.x, ps.y, ps.heading, ps.kappa, ps.part, ps.gear) for ps, *_ in sets], _sample_columns(), dev)
    i64 = lambda ts: torch.cat(ts) if ts else torch.zeros(0, dtype=torch.int64, device=dev)
    per_item = lambda value, o: torch.full((int(o.numel()),), int(value), dtype=torch.int64, device=dev)
    order, ioff = _group_by(i64([f[o] for _, f, _, o in sets]), n, 'an item names a field outside 0 .. n_fields - 1')
    ipath = i64([o + int(first[k]) for k, (*_, o) in enumerate(sets)])[order].contiguous()
    iset = i64([per_item(k, o) for k, (*_, o) in enumerate(sets)])[order].to(torch.int32)
    iclosed = i64([per_item(closed, o) for _, _, closed, o in sets])[order].to(torch.int32).contiguous()
    ipath_h = ipath.cpu().numpy()
    poff_h = poff.cpu().numpy() if poff_h is None else poff_h
    lens = poff_h[1:] - poff_h[:-1]
    longest = int(lens[ipath_h[iclosed.cpu().numpy() != 0]].max()) if len(ipath_h) and bool((iclosed != 0).any()) else 0
    return _MissionTable(n, first, starts, PathSet(poff, poff_h, *cols), ioff, ioff.cpu().numpy(), ipath, ipath_h, iset, iclosed, longest)


def mission_paths(items, radius, spacing, reversing=False, entry=None, exit=None, station_step=None, device=None, innermost_first=False,
                  n_fields=None, clear_of=None):
    """ONE drivable path per field from its path sets (fcpp_mission_solve + _counts + _fill; the rule: include/fcpp.h) -> MissionPaths.
    items: a sequence, in DRIVING ORDER, of FieldPaths (open, path i belongs to field i), HeadlandPaths (closed loops, field =
    ring_pair[:, 0]; its rings in stored order, or the innermost pass first with innermost_first=True) or tuples (offsets, x, y, heading,
    kappa, part, gear, field, closed).  A field's items are ordered by (position in `items`, path order within the set).  Consecutive
    items, and the entry / exit pose (one (x, y, heading) per field), are joined by the shortest Dubins path -- Reeds-Shepp if `reversing`
    -- planned at _chord_radius(radius, spacing) as the field paths plan; every closed loop is entered at the station that makes the joints
    shortest in all, driven for one lap and left there.  Stations: every max(1, round(station_step / set spacing))-th sample of a loop
    that lies on a straight element or a followed arc; by default the stride that gives the longest loop at most 128 stations.  A loop of
    more than FCPP_MISSION_MAX_STATIONS stations fails its field (status FCPP_EUNSUPPORTED: raise station_step).  The ORDER of the items is
    the caller's; joints know no boundary (validate() flags what leaves the field) -- with clear_of (one region per field) the chosen joints
    are run through clear_connectors and `blocked` counts, per field, those without a clear word; the stations stay chosen by the plain
    lengths."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    items = list(items)
    t = _mission_table(items, dev, innermost_first, n_fields, entry, exit)
    n, n_items, ps = t.n, len(t.ipath_h), t.paths
    if station_step is None:
        stride = max(1, -(-(t.longest - 1) // 128))
    else:
        if not float(station_step) > 0.0:
            raise ValueError('station_step must be positive')
        set_spacing = next((s for s in (getattr(st, 'spacing', None) for st in items) if s), spacing)
        stride = max(1, int(round(float(station_step) / float(set_spacing))))
    R, mode = _chord_radius(radius, spacing), 1 if reversing else 0
    ent, ext = _pose_columns(entry, n, dev), _pose_columns(exit, n, dev)
    n_slots = 2 * n_items + n if n else 0
    status = torch.empty(n, dtype=torch.int32, device=dev)
    transit = torch.empty(n, dtype=torch.float64, device=dev)
    skipped = torch.empty(n, dtype=torch.int32, device=dev)
    # (a failed field's per-item and per-slot rows are not written: they keep these values)
    station = torch.full((n_items,), -1, dtype=torch.int64, device=dev)
    slot_item = torch.full((n_slots,), -1, dtype=torch.int64, device=dev)
    slot_word = torch.full((n_slots,), -1, dtype=torch.int32, device=dev)
    slot_seg = torch.full((n_slots, 5), float('nan'), dtype=torch.float64, device=dev)
    slot_total = torch.full((n_slots,), float('nan'), dtype=torch.float64, device=dev)
    head = (mode, n, _ptr(t.ioff), _host_ptr(t.ioff_h), n_items, _ptr(t.ipath), _host_ptr(t.ipath_h), _ptr(t.iclosed), int(t.first[-1]), _ptr(ps.offsets),
            _host_ptr(ps.offsets_host), int(t.starts[-1]))
    rec = (_ptr(status), _ptr(station), _ptr(slot_item), _ptr(slot_word), _ptr(slot_seg))
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_mission_solve(ctx.handle, *head, _ptr(ps.x), _ptr(ps.y), _ptr(ps.heading), _ptr(ps.part), _ptr(ps.gear), *[_ptr(c) for c in ent],
                                       *[_ptr(c) for c in ext], R, stride, _ptr(status), _ptr(transit), _ptr(skipped), _ptr(station), _ptr(slot_item),
                                       _ptr(slot_word), _ptr(slot_seg), _ptr(slot_total)))
    slot_off = torch.empty(n_slots + 1, dtype=torch.int64, device=dev)
    *samples, osrc = _counts_fill(
        n, dev, lambda off, off_h: ctx.lib.fcpp_mission_counts(ctx.handle, *head, *rec, float(spacing), off, off_h, _ptr(slot_off)),
        lambda off, off_h, total, *cols: ctx.lib.fcpp_mission_fill(ctx.handle, *head, _ptr(ps.x), _ptr(ps.y), _ptr(ps.heading), _ptr(ps.kappa),
                                                                   _ptr(ps.part), _ptr(ps.gear), *[_ptr(c) for c in ent], R, float(spacing), *rec,
                                                                   _ptr(slot_off), total, *cols), _sample_columns(torch.int32, torch.int64))
    src_set = (torch.searchsorted(torch.as_tensor(t.starts[1:], device=dev), osrc, right=True).to(torch.int32)
               if len(items) else torch.zeros(int(osrc.numel()), dtype=torch.int32, device=dev))
    src_set = torch.where(osrc >= 0, src_set, torch.full((), -1, dtype=torch.int32, device=dev))
    mp = MissionPaths(*samples, osrc, src_set, status, transit, skipped, t.ioff, t.ipath, t.iclosed, t.iset, station, slot_off, slot_item, slot_word,
                      slot_seg, slot_total, float(R), bool(reversing), int(stride), t.starts)
    mp._sets = tuple(items)
    if clear_of is not None:
        mp.blocked = _mission_blocked(mp, _clear_fields(clear_of, n, device), ent, ext, device)
    return mp


def _mission_blocked(mp, pf, ent, ext, device):
    """the chosen joints through clear_connectors against their field's region -> per field the joints without a clear word"""
    torch = _torch()
    dev = mp.x.device
    n = int(mp.offsets.numel()) - 1
    blocked = torch.zeros(n, dtype=torch.int32, device=dev)
    joint = torch.nonzero(mp.slot_word >= 0).reshape(-1)
    if int(joint.numel()) == 0:
        return blocked
    first = 2 * mp.item_offsets + torch.arange(n + 1, dtype=torch.int64, device=dev)
    f = torch.searchsorted(first, joint, right=True) - 1
    a, b = mp.slot_offsets[joint], mp.slot_offsets[joint + 1]
    total = int(mp.x.numel())
    sample = torch.stack([mp.x, mp.y, mp.heading], dim=1)
    pose = lambda cols: torch.stack(cols, dim=1)[f] if cols[0] is not None else torch.zeros((int(f.numel()), 3), dtype=torch.float64, device=dev)
    at_entry, at_exit = (joint == first[f]).unsqueeze(1), (b == mp.offsets[f + 1]).unsqueeze(1)
    frm = torch.where(at_entry, pose(ent), sample[(a - 1).clamp(min=0)])
    to = torch.where(at_exit, pose(ext), sample[b.clamp(max=total - 1)])
    cc = clear_connectors(frm, to, pf, f, mp.radius, reversing=mp.reversing, device=device)
    blocked.index_add_(0, f, (cc.rank < 0).to(torch.int32))
    return blocked


# ---- polygon coverage (fcpp_polygon_cover_sizes / fcpp_polygon_cover; the rule: include/fcpp.h) -----------------------------------------
@dataclass
class PolygonCoverage:
    """polygon_coverage(): what the working passes of a path set cover of every field, on a grid of res x res cells"""
    counts: object              # (n, 4) int64, device: cells inside; inside and covered; inside and overlapped; covered and not inside
    res: float
    status: object              # (n) int32: 0, FCPP_EINVAL (the swath rule) or FCPP_EUNSUPPORTED (more than 2^28 cells): no cells, zero counts
    dims: object                # (n, 4) int64, device: gx, gy (float64 bits: origin()), nx, ny
    cell_offsets: object        # (n + 1) int64, device; cell_offsets_host: the numpy copy
    cell_offsets_host: object
    cells: object = None        # (total cells) uint8 when asked for (want_grid): bit 0 inside, bit 1 covered, bit 2 overlapped

    def _area(self, k):
        return self.counts[:, k].to(_torch().float64) * (self.res * self.res)

    @property
    def field_area(self):
        return self._area(0)

    @property
    def covered_area(self):
        return self._area(1)

    @property
    def missed_area(self):
        return self._area(0) - self._area(1)

    @property
    def overlap_area(self):
        return self._area(2)

    @property
    def spill_area(self):
        return self._area(3)

    @property
    def rate(self):
        """covered / inside per field; NaN for a field without cells"""
        f64 = _torch().float64
        return self.counts[:, 1].to(f64) / self.counts[:, 0].to(f64)

    def origin(self):
        """(n, 2) float64: gx, gy -- cell (a, b) of field i is sampled at origin[i] + (a + 0.5, b + 0.5) res"""
        return self.dims[:, :2].contiguous().view(_torch().float64)

    def grid(self, i):
        """field i's cells as an (ny, nx) view (want_grid=True)"""
        if self.cells is None:
            raise ValueError('polygon_coverage(..., want_grid=True) keeps the cells')
        nx, ny = (int(v) for v in self.dims[i, 2:].tolist())
        return self.cells[int(self.cell_offsets_host[i]):int(self.cell_offsets_host[i + 1])].view(ny, nx)

    def regions(self, **kw):
        """coverage_regions(self, **kw): the connected patches of one kind of cell (want_grid=True)"""
        return coverage_regions(self, **kw)


def _cover_set(ps, first_path, dev):
    """polygon_coverage's normaliser: a PathSet, or the tuple (offsets, x, y, path_field, work, pass) -> (PathSet -- of a tuple only its
    offsets, x and y --, path_field int64, work uint8, pass int32), all on the device"""
    torch = _torch()
    if isinstance(ps, PathSet):
        return ps, ps.path_field(), ps.work().to(torch.uint8), ps.pass_id()
    offsets, x, y, path_field, work, pas = ps
    x, y = _dev_f64(x, dev).reshape(-1), _dev_f64(y, dev).reshape(-1)
    total = int(x.numel())
    off, off_h = _offsets(offsets, total, dev)
    np_ = int(off.numel()) - 1
    pf = torch.zeros(np_, dtype=torch.int64, device=dev) if path_field is None else torch.as_tensor(path_field, device=dev).to(torch.int64).reshape(-1)
    w = torch.ones(total, dtype=torch.uint8, device=dev) if work is None else (torch.as_tensor(work, device=dev).reshape(-1) != 0).to(torch.uint8)
    pas = first_path + _owners(off, total, torch.int32) if pas is None else torch.as_tensor(pas, device=dev).to(torch.int32).reshape(-1)
    if int(pf.numel()) != np_ or int(w.numel()) != total or int(pas.numel()) != total or int(y.numel()) != total:
        raise ValueError('a path set needs one field per path and one work flag and pass id per sample')
    return PathSet(off, off_h, x, y, None, None, None, None), pf, w, pas


def _cover_paths(paths, n, dev):
    """the path sets of polygon_coverage, joined on the device -> (n_paths, total, path_offsets, its host copy or None, x, y, work, pass,
    field_path_offsets, path_ids): what fcpp_polygon_cover takes"""
    torch = _torch()
    if isinstance(paths, PathSet) or (isinstance(paths, tuple) and len(paths) == 6 and not isinstance(paths[0], (PathSet, tuple))):
        paths = (paths,)          # (one set, itself or as a tuple, not a sequence of sets)
    sets, n_paths = [], 0
    for ps in paths:
        sets.append(_cover_set(ps, n_paths, dev))
        n_paths += int(sets[-1][0].offsets.numel()) - 1
    _, starts, poff, poff_h, (x, y, work, pas) = _join_csr([ps.offsets for ps, *_ in sets], [ps.offsets_host for ps, *_ in sets],
                                                           [(ps.x, ps.y, w, p) for ps, _, w, p in sets],
                                                           (torch.float64, torch.float64, torch.uint8, torch.int32), dev)
    owner = torch.cat([f.to(dev) for _, f, _, _ in sets]) if sets else torch.zeros(0, dtype=torch.int64, device=dev)
    ids, fpo = _group_by(owner, n, 'path_field must name a field of the batch')
    return n_paths, int(starts[-1]), poff, poff_h, x, y, work, pas, fpo, ids


def polygon_coverage(fields, width, res, paths=(), caps='flat', want_grid=False, device=None):
    """The coverage report of a batch of polygon fields (fcpp_polygon_cover_sizes + fcpp_polygon_cover) -> PolygonCoverage.  `fields` are the
    SURVEYED boundaries (what headland() was given, not the work area), `width` the working width, `res` the cell size [m].  paths: one or
    more FieldPaths / HeadlandPaths, or tuples (offsets, x, y, path_field, work, pass) -- path_field: the field of every path (None: field
    0), work: a flag per sample (None: all work), pass: an id per sample (None: the path's index); they are concatenated on the device.
    Only the working samples cover: the swaths of field paths (pass id: the leg), the straight elements and followed arcs of headland loops
    (one id per ring, negative: distinct from the legs).  A cell is covered iff a working segment passes within width / 2 of its centre,
    runs ending flat (caps='flat') or round ('round': fcpp_cover_grid's predicate), overlapped iff segments of two different pass ids do.
    Per field: counts, field_area, covered_area, missed_area, overlap_area, spill_area (covered outside the boundary or inside a hole), rate;
    want_grid=True keeps the cells (grid(i))."""
    ctx = get_context(device)
    torch = _torch()
    pf = polygon_fields(fields, device)
    dev = pf.x.device
    n = pf.n
    if caps not in ('flat', 'round'):
        raise ValueError("caps must be 'flat' or 'round'")
    n_paths, total, poff, poff_h, x, y, work, pas, fpo, ids = _cover_paths(paths, n, dev)
    dims = torch.empty((n, 4), dtype=torch.int64, device=dev)
    coff, coff_h = torch.empty(n + 1, dtype=torch.int64, device=dev), np.zeros(n + 1, dtype=np.int64)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty((n, 4), dtype=torch.int64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_polygon_cover_sizes(ctx.handle, *pf._head(), float(width), float(res), _ptr(dims), _ptr(coff), _host_ptr(coff_h), _ptr(status)))
    cells = torch.empty(int(coff_h[-1]), dtype=torch.uint8, device=dev) if want_grid else None
    L.check(ctx.lib.fcpp_polygon_cover(ctx.handle, *pf._head(), float(width), float(res), 1 if caps == 'round' else 0, n_paths, _ptr(poff),
                                       _host_ptr(poff_h), total, _ptr(x), _ptr(y), _ptr(work), _ptr(pas), _ptr(fpo), _ptr(ids), _ptr(coff),
                                       _host_ptr(coff_h), _ptr(cells), _ptr(counts), _ptr(status)))
    return PolygonCoverage(counts, float(res), status, dims, coff, coff_h, cells)


# ---- coverage regions (fcpp_cover_regions_counts / _fill; the rule: include/fcpp.h) -----------------------------------------------------
REGION_KINDS = {'missed': (3, 1), 'overlapped': (4, 4), 'spill': (3, 2), 'covered': (3, 3)}


@dataclass
class CoverageRegions:
    """coverage_regions(): the connected patches of one kind of cell of every field, in ascending key (smallest cell index) per field"""
    offsets: object             # (n + 1) int64, device: field i's KEPT regions are offsets[i] .. offsets[i + 1]; offsets_host: the numpy copy
    offsets_host: object
    first: object               # (k) int64: the region's key, its smallest field-local cell index b nx + a
    cells: object               # (k) int64
    bbox: object                # (k, 4) int32: a_min, a_max, b_min, b_max
    sums: object                # (k, 2) int64: the sums of the members' column and row indices
    area: object                # (k) float64: cells res^2 [m^2]
    centroid: object            # (k, 2) float64, world metres: gx + (sum_a / cells + 0.5) res, likewise in y
    bounds: object              # (k, 4) float64, world metres: x_min, y_min, x_max, y_max of the region's cells (gx + a_min res .. gx + (a_max + 1) res)
    dropped: object             # (n, 2) int64: the regions below min_area that were left out, and their cells
    kind: object                # the name, or the (mask, value) pair
    connectivity: int
    coverage: object            # the PolygonCoverage the regions are of
    labels: object = None       # (total cells) int32 when asked for (want_labels): the index of the cell's region among its field's KEPT regions, -1 for a non-member, -2 for a cell of a dropped region

    def field(self, i):
        """the slice of field i's regions in first .. bounds"""
        return slice(int(self.offsets_host[i]), int(self.offsets_host[i + 1]))

    def label_grid(self, i):
        """field i's labels as an (ny, nx) view (want_labels=True)"""
        if self.labels is None:
            raise ValueError('coverage_regions(..., want_labels=True) keeps the labels')
        cov = self.coverage
        nx, ny = (int(v) for v in cov.dims[i, 2:].tolist())
        return self.labels[int(cov.cell_offsets_host[i]):int(cov.cell_offsets_host[i + 1])].view(ny, nx)


def coverage_regions(coverage, kind='missed', connectivity=4, min_area=0.0, want_labels=False, device=None):
    """The connected regions of one kind of cell in a PolygonCoverage made with want_grid=True (fcpp_cover_regions_counts + _fill) ->
    CoverageRegions.  kind: 'missed' (inside and not covered), 'overlapped', 'spill' (covered and not inside), 'covered', or a
    (mask, value) pair: cell c is a member iff (cells[c] & mask) == value.  connectivity 4 or 8; neighbours exist only inside one field's
    grid.  The device labels and numbers EVERY region; min_area [m^2] then filters the records (not the cells): the kept regions keep
    their order, `dropped` says per field how many regions and cells were left out, and with want_labels the label grid is renumbered to
    the kept regions (-2 for a cell of a dropped one)."""
    torch = _torch()
    if coverage.cells is None:
        raise ValueError('coverage_regions needs the cells: polygon_coverage(..., want_grid=True)')
    if isinstance(kind, str):
        if kind not in REGION_KINDS:
            raise ValueError('kind must be one of %s or a (mask, value) pair' % ', '.join(sorted(REGION_KINDS)))
        mask, value = REGION_KINDS[kind]
    else:
        mask, value = (int(v) for v in kind)
    if connectivity not in (4, 8):
        raise ValueError('connectivity must be 4 or 8')
    dev = coverage.cells.device
    ctx = get_context(dev.index if device is None else device)
    n = int(coverage.dims.shape[0])
    dims, coff = coverage.dims.contiguous(), coverage.cell_offsets.contiguous()
    coff_h = np.ascontiguousarray(coverage.cell_offsets_host, dtype=np.int64)
    total = int(coff_h[-1])
    labels = torch.empty(total, dtype=torch.int32, device=dev)
    roff, roff_h = torch.empty(n + 1, dtype=torch.int64, device=dev), np.zeros(n + 1, dtype=np.int64)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_cover_regions_counts(ctx.handle, n, _ptr(dims), _ptr(coff), _host_ptr(coff_h), _ptr(coverage.cells), mask, value,
                                              int(connectivity), _ptr(labels), _ptr(roff), _host_ptr(roff_h)))
    k = int(roff_h[-1])
    rec = torch.empty((k, 6), dtype=torch.int64, device=dev)          # 48 bytes per record
    L.check(ctx.lib.fcpp_cover_regions_fill(ctx.handle, n, _ptr(dims), _ptr(coff), _host_ptr(coff_h), _ptr(labels), _ptr(roff), _host_ptr(roff_h), k,
                                            _ptr(rec)))
    res = float(coverage.res)
    field_of = _owners(roff, k)
    dropped = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    if min_area > 0.0:
        keep = rec[:, 1].to(torch.float64) * (res * res) >= float(min_area)
        gone = ~keep
        dropped[:, 0].index_add_(0, field_of, gone.to(torch.int64))
        dropped[:, 1].index_add_(0, field_of, torch.where(gone, rec[:, 1], torch.zeros_like(rec[:, 1])))
        kept_before = torch.cumsum(keep.to(torch.int64), dim=0) - keep.to(torch.int64)
        new_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        new_off[1:] = torch.cumsum(torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, field_of, keep.to(torch.int64)), dim=0)
        if want_labels and k:
            # one gather: a region's new index within its field, -2 when it was dropped; slot k serves the non-members
            remap = torch.cat([torch.where(keep, kept_before - new_off[field_of], torch.full_like(kept_before, -2)),
                               torch.full((1,), -1, dtype=torch.int64, device=dev)]).to(torch.int32)
            slot = torch.where(labels >= 0, labels.to(torch.int64) + roff[_owners(coff, total)], torch.full((1,), k, dtype=torch.int64, device=dev))
            labels = remap[slot]
        rec, field_of, roff = rec[keep], field_of[keep], new_off
        roff_h = roff.cpu().numpy()
    org = coverage.origin()[field_of]                                   # (k, 2)
    box = rec[:, 2:4].contiguous().view(torch.int32).reshape(-1, 4)
    cells = rec[:, 1]
    sums = rec[:, 4:6].contiguous()
    f64 = torch.float64
    centroid = org + (sums.to(f64) / cells.to(f64).unsqueeze(1) + 0.5) * res
    lo = torch.stack([box[:, 0], box[:, 2]], dim=1).to(f64)
    hi = torch.stack([box[:, 1], box[:, 3]], dim=1).to(f64) + 1.0
    bounds = torch.cat([org + lo * res, org + hi * res], dim=1)
    return CoverageRegions(roff, roff_h, rec[:, 0].contiguous(), cells.contiguous(), box, sums, cells.to(f64) * (res * res), centroid, bounds, dropped,
                           kind, int(connectivity), coverage, labels if want_labels else None)


# ---- patch passes (fcpp_patch_sizes / _counts / _fill; the rule: include/fcpp.h) ---------------------------------------------------------
@dataclass
class PatchInfo:
    """patch_swaths(): what the patch passes know beyond a SwathSet"""
    region: object              # (m) int64: the global index (into the CoverageRegions' records) of every swath's region
    n_lines: object             # (k) int64: the lines K of every region
    n_bins: object              # (k) int64: the bins B along each of its lines
    status: object              # (k) int32: 0, or FCPP_EUNSUPPORTED (more than 2^22 lines, or 2^31 bitmap words or more): no swaths
    frame: object               # (n, 2) float64: sin and cos of every field's track angle
    records: object             # (k, 8) int64: the 64-byte records as the library wrote them (u_min, w_lo as float64 bits, K, B, first line, first word, status, u_max)
    margin: float
    join: float


def patch_swaths(regions, width, angle, margin=None, join=None, device=None):
    """Straight working passes over every kept region of a CoverageRegions made with want_labels=True (fcpp_patch_sizes + _counts + _fill)
    -> (SwathSet, PatchInfo).  The passes lie parallel to the field's tracks -- `angle` is a scalar or one value per field -- in strips of
    width - 2 margin across them, centred on the region's extent; along a line they reach from the first to the last cell of every run of
    cells, `margin` beyond both, and runs less than `join` metres apart are driven as one.  margin defaults to res / 2 (at angle 0 the
    whole cell squares are covered), join to `width`.  Every member cell lies within (width - 2 margin) / 2 of its line and at least
    `margin` inside a swath's ends.  The SwathSet is an ordinary one (route_swaths, field_paths, polygon_coverage take it): its status is 0
    for every field, n_lines the lines of all the field's regions; a region the rule does not support (PatchInfo.status) has no swaths.
    Out of scope: shifting a line inward where a sliver along the boundary makes the pass spill outside (a second polygon_coverage reports
    the spill), an angle per region, clipping against holes beyond what `join` decides."""
    torch = _torch()
    if regions.labels is None:
        raise ValueError('patch_swaths needs the labels: coverage_regions(..., want_labels=True)')
    cov = regions.coverage
    dev = regions.labels.device
    ctx = get_context(dev.index if device is None else device)
    n = int(cov.dims.shape[0])
    res = float(cov.res)
    margin = res / 2 if margin is None else float(margin)
    join = float(width) if join is None else float(join)
    ang = _one_per(_dev_f64(angle, dev), n, 'angle', 'value per field')
    dims, coff, labels, roff = cov.dims.contiguous(), cov.cell_offsets.contiguous(), regions.labels.contiguous(), regions.offsets.contiguous()
    coff_h = np.ascontiguousarray(cov.cell_offsets_host, dtype=np.int64)
    roff_h = np.ascontiguousarray(regions.offsets_host, dtype=np.int64)
    k = int(roff_h[-1])
    i64 = torch.int64
    frame = torch.empty((n, 2), dtype=torch.float64, device=dev)
    rec = torch.empty((k, 8), dtype=i64, device=dev)                 # 64 bytes per record
    totals = np.zeros(2, dtype=np.int64)
    rule = (float(width), margin, join)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_patch_sizes(ctx.handle, n, _ptr(dims), _ptr(coff), _host_ptr(coff_h), res, _ptr(labels), _ptr(roff), _host_ptr(roff_h), k,
                                     _ptr(ang), *rule, _ptr(frame), _ptr(rec), _host_ptr(totals)))
    n_lines, n_words = int(totals[0]), int(totals[1])
    bitmap, cnt = torch.empty(n_words, dtype=i64, device=dev), torch.empty(n_lines, dtype=i64, device=dev)
    loff, soff = torch.empty(n_lines + 1, dtype=i64, device=dev), torch.empty(n + 1, dtype=i64, device=dev)
    soff_h = np.zeros(n + 1, dtype=np.int64)
    L.check(ctx.lib.fcpp_patch_counts(ctx.handle, n, _ptr(dims), _ptr(coff), _host_ptr(coff_h), res, _ptr(labels), _ptr(roff), _host_ptr(roff_h), k,
                                      _ptr(frame), *rule, _ptr(rec), n_lines, n_words, _ptr(bitmap), _ptr(cnt), _ptr(loff), _ptr(soff),
                                      _host_ptr(soff_h)))
    m = int(soff_h[-1])
    a, b = torch.empty((2, m), dtype=torch.float64, device=dev), torch.empty((2, m), dtype=torch.float64, device=dev)
    line, length = torch.empty(m, dtype=torch.int32, device=dev), torch.empty(m, dtype=torch.float64, device=dev)
    region = torch.empty(m, dtype=i64, device=dev)
    L.check(ctx.lib.fcpp_patch_fill(ctx.handle, n, _ptr(dims), res, _ptr(roff), _host_ptr(roff_h), k, _ptr(frame), *rule, _ptr(rec), n_lines, n_words,
                                    _ptr(bitmap), _ptr(loff), m, _ptr(a[0]), _ptr(a[1]), _ptr(b[0]), _ptr(b[1]), _ptr(line), _ptr(length), _ptr(region)))
    lines_of_field = torch.zeros(n, dtype=i64, device=dev).index_add_(0, _owners(roff, k), rec[:, 2]).to(torch.int32)
    status = rec[:, 6].contiguous().view(torch.int32).reshape(-1, 2)[:, 0].contiguous()
    ss = SwathSet(soff, soff_h, a.t().contiguous(), b.t().contiguous(), line, length, torch.zeros(n, dtype=torch.int32, device=dev), lines_of_field, ang)
    return ss, PatchInfo(region, rec[:, 2].contiguous(), rec[:, 3].contiguous(), status, frame, rec, margin, join)


# ---- path speeds (fcpp_path_speeds; the rule: include/fcpp.h) -----------------------------------------------------------------------------
@dataclass
class PathSpeeds:
    """path_speeds(): the speed of every sample of a path set, in the units and CSR form trajectory(), validate() and trajectory_sample()
    take.  Path p owns the samples offsets[p] .. offsets[p + 1]."""
    v: object                   # (total) float64 [km/h]: the greatest profile under the caps and the two acceleration limits; 0 at a stop
    cap: object                 # (total) float64 [km/h]: the pointwise cap, 0 at a stop
    status: object              # (n) int32: 0, or FCPP_EINVAL (a sample that is not finite, a part outside 0 .. 7, a gear other than +-1): v and cap NaN
    offsets: object             # (n + 1) int64, device; offsets_host: the numpy copy or None
    offsets_host: object
    x: object = None            # the path set's columns the speeds belong to (what trajectory() below reads)
    y: object = None
    gear: object = None
    params: object = None       # the L.SpeedParams of the call

    def trajectory(self):
        """trajectory() of the paths at these speeds, the gear -1 samples flagged FCPP_KIND_REVERSE so that the headings are the vehicle's
        -> (s, t, heading, totals); totals[p] = (length, time) of path p"""
        fs = (self.gear < 0).to(_torch().int32) * L.KIND_REVERSE
        return trajectory(self.x, self.y, self.v, flagseg=fs, offsets=self.offsets if self.offsets_host is None else self.offsets_host,
                          device=self.v.device.index)


def speed_params(vehicle, reverse_kmh=2.5, turn_kmh=None, a_dec=None, rest_start=True, rest_end=True, stop_at_cusps=True, nominal=None):
    """L.SpeedParams from a vehicle: parts 0 and 4 work at max_work_speed_kmh, parts 1, 2, 3, 5, 6 (and the spare 7) drive at
    max_headland_speed_kmh (nominal: eight values by part instead); turn_kmh = headland_turn_speed_kmh; a_acc = max_longitudinal_accel and
    a_dec likewise unless given; a_lat, safety_factor and kappa_eps = 1e-6 as the reference has them (MLP:496-499); reverse_kmh: MLP:1080"""
    p = L.SpeedParams()
    if nominal is None:
        nominal = [vehicle.max_work_speed_kmh if k in (0, 4) else vehicle.max_headland_speed_kmh for k in range(8)]
    if len(nominal) != 8:
        raise ValueError('nominal takes eight speeds, one per part 0 .. 7')
    for k in range(8):
        p.nominal_kmh[k] = float(nominal[k])
    p.reverse_kmh = float(reverse_kmh)
    p.turn_kmh = float(vehicle.headland_turn_speed_kmh if turn_kmh is None else turn_kmh)
    p.a_lat, p.safety_factor, p.kappa_eps = vehicle.max_lateral_accel, vehicle.safety_factor, 1e-6
    p.a_acc = vehicle.max_longitudinal_accel
    p.a_dec = float(vehicle.max_longitudinal_accel if a_dec is None else a_dec)
    p.flags = (L.SPEED_REST_START if rest_start else 0) | (L.SPEED_REST_END if rest_end else 0) | (L.SPEED_STOP_AT_CUSPS if stop_at_cusps else 0)
    return p


def path_speeds(paths, vehicle, reverse_kmh=2.5, turn_kmh=None, a_dec=None, rest_start=True, rest_end=True, stop_at_cusps=True, nominal=None,
                device=None):
    """The speed profile of sampled paths (fcpp_path_speeds) -> PathSpeeds.  paths: a FieldPaths, HeadlandPaths, TransitPaths or
    MissionPaths, or a tuple (offsets, x, y, kappa, part, gear).  Caps from part, gear and the stored kappa (speed_params() says which);
    the vehicle stands at every Reeds-Shepp cusp (stop_at_cusps) and at the path ends (rest_start, rest_end); in between the greatest
    profile that speeds up by at most max_longitudinal_accel and brakes by at most a_dec."""
    torch = _torch()
    if isinstance(paths, (tuple, list)):          # (the tuple form as a PathSet: its columns as given, no heading)
        offsets, x, y, kappa, part, gear = paths
        paths = PathSet(offsets, None, x, y, None, kappa, part, gear)
    offsets, x, y, kappa, part, gear = paths.offsets if paths.offsets_host is None else paths.offsets_host, paths.x, paths.y, paths.kappa, paths.part, paths.gear
    if device is None and isinstance(x, torch.Tensor) and x.is_cuda:
        device = x.device.index
    ctx = get_context(device)
    dev = torch.device('cuda', ctx.device)
    x, y, kappa = _dev_f64(x, dev), _dev_f64(y, dev), _dev_f64(kappa, dev)
    i8 = lambda a: (a.to(device=dev, dtype=torch.int8).contiguous() if isinstance(a, torch.Tensor)
                    else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int8), device=dev))
    part, gear = i8(part), i8(gear)
    total = x.numel()
    if not (y.numel() == kappa.numel() == part.numel() == gear.numel() == total):
        raise ValueError('x, y, kappa, part and gear hold one value per sample')
    off, off_h = _offsets(offsets, total, dev)
    n = off.numel() - 1
    prm = speed_params(vehicle, reverse_kmh, turn_kmh, a_dec, rest_start, rest_end, stop_at_cusps, nominal)
    v, cap = torch.empty_like(x), torch.empty_like(x)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_path_speeds(ctx.handle, C.byref(prm), n, _ptr(off), total, _ptr(x), _ptr(y), _ptr(kappa), _ptr(part), _ptr(gear), _ptr(v),
                                     _ptr(cap), _ptr(status), _host_ptr(off_h)))
    return PathSpeeds(v, cap, status, off, off_h, x, y, gear, prm)


_drive_headland = headland_paths      # (plan_polygon_fields has a flag of that name)


@dataclass
class PolygonPlan:
    """plan_polygon_fields(): every stage's result for the batch"""
    headland: object            # InsetSet: the centre lines of the headland passes
    work: object                # PolygonFields: the work areas
    angle_index: object         # (n) int64: the chosen index into `angles`, -1 where no angle is valid
    angle: object               # (n) float64: the track angle driven
    swaths: object              # SwathSet
    route: object               # SwathRoute
    paths: object               # FieldPaths
    headland_paths: object = None       # HeadlandPaths of `headland` when asked for (headland_paths=True), else None
    coverage: object = None             # PolygonCoverage of `fields` under paths (and headland_paths) when asked for (coverage_resolution), else None
    clearance: object = None            # FieldPathClearance of `paths` against clear_of when given, else None
    transits: object = None             # LoopTransits of the rank -1 legs of `paths` when asked for (detour=True), else None
    missed: object = None               # CoverageRegions of the missed cells of `coverage` when asked for (missed_min_area), else None
    patch: object = None                # SwathSet of the patch passes over `missed` when asked for (patch=True), else None
    patch_info: object = None           # PatchInfo of `patch`
    patch_paths: object = None          # FieldPaths over `patch`, routed per field
    coverage_after: object = None       # PolygonCoverage of `fields` under the plan's paths AND patch_paths, its cells kept
    mission: object = None              # MissionPaths: loops, field path and patch passes joined into one drive per field (mission=...), else None
    speeds: object = None               # PathSpeeds of `mission` when there is one, else of `paths` (speeds=vehicle), else None


def plan_polygon_fields(fields, width, radius, spacing, angles, passes=1, turn_cost=0.0, reversing=False, starts=8, entry=None, exit=None,
                        arc_step=0.1, headland_paths=False, coverage_resolution=None, device=None, clear_of=None, reshape=False,
                        price_clear=False, detour=False, missed_min_area=None, patch=False, mission=None, speeds=None):
    """The whole chain for a batch of polygon fields, every stage one batched call on the device: headland(passes) -> best_swath_angle over
    `angles` -> polygon_swaths at each field's best angle -> route_swaths(spacing=spacing) -> field_paths.  -> PolygonPlan.  A field whose
    work area is empty, or for which no angle is valid, carries its stage's status (swaths.status) and has no samples; the rest is planned.
    The headland pass rings are returned (headland) but not part of the path; headland_paths=True also drives them (headland_paths() at the
    same radius, spacing and `reversing`: one closed loop per ring, PolygonPlan.headland_paths).  The loops are joined to each other and
    to the field paths by mission= (below).  coverage_resolution [m]: also report what the
    plan covers of the ORIGINAL fields (polygon_coverage at that cell size over the field paths, and the headland loops if they were driven:
    PolygonPlan.coverage); nothing else in the chain changes.  clear_of: None leaves the plan as it is; 'boundary' routes the swaths so
    that the connectors stay clear of the surveyed `fields` (holes are ponds) where an order allows it, and reports what stays blocked
    (route_swaths(clear_of=...): PolygonPlan.clearance is its SwathRoute.clearance, what field_path_clearance gives for the path); a PolygonFields, or anything polygon_fields takes, is used
    as given.  reshape=True (with clear_of; ValueError without): the field paths drive, per connector, the shortest word that stays off the
    same region the router was given (field_paths(clear_of=...)): PolygonPlan.paths.blocked / .reshaped report the path as driven, while
    PolygonPlan.clearance stays what it is, the shortest-word legs as routed.  price_clear=True (with reshape=True; ValueError without:
    the route would be priced with words nobody drives): the router's matrix holds the clear words' lengths
    (route_swaths(price_clear=True)), so route.length is paths.transit_length and route.blocked is paths.blocked.  The headland loops'
    corner connectors are neither tested nor re-shaped.  detour=True (with reshape=True and headland_paths=True; ValueError without): the
    legs for which no word is clear ride the plan's own headland loops, driven in both directions, round the obstacle
    (field_paths(loops=...)): PolygonPlan.transits is paths.transits, paths.blocked the legs that stay blocked, paths.detoured those that
    ride.  The router does not price the transits: route.length then differs from paths.transit_length on a detoured field.
    missed_min_area [m^2] (with coverage_resolution; ValueError without): the coverage keeps its cells and PolygonPlan.missed holds the
    connected missed patches of at least that area (coverage_regions(kind='missed', min_area=...)); None: the chain makes exactly the calls
    it makes without it.
    patch=True (with missed_min_area; ValueError without): the missed regions keep their labels, patch_swaths lays passes over them at
    each field's chosen angle (PolygonPlan.patch, .patch_info), route_swaths + field_paths drive them at the same radius, spacing and
    `reversing` (.patch_paths), and a second polygon_coverage over the plan's path sets plus the patch paths -- their pass ids are
    leg + 2^30, apart from the first set's legs and the rings' negative ids -- says what is covered then (.coverage_after, cells kept).
    The patch paths are joined to the field path by mission=; patch=False: the chain makes exactly the calls it makes without it.
    mission='headland_first' | 'headland_last' (with headland_paths=True; ValueError without): ONE drivable path per field
    (mission_paths(): PolygonPlan.mission), gate -> loops -> swaths -> patch passes -> gate.  'headland_first' drives the passes outermost
    -> innermost, then `paths`, then patch_paths if present; 'headland_last' drives `paths`, the patch paths, then the passes innermost ->
    outermost.  entry / exit then belong to the MISSION: the router still prices them, the field paths are built without them.  With
    clear_of the chosen joints are tested against the same region (mission.blocked).  None: the chain makes exactly the calls it makes
    without it.
    speeds=vehicle: the speed of every sample of the drive (path_speeds() at its defaults for that vehicle: PolygonPlan.speeds) -- of
    `mission` when there is one, else of `paths`; its trajectory() gives time stamps and totals.  None: the chain makes exactly the calls
    it makes without it."""
    if mission not in (None, 'headland_first', 'headland_last'):
        raise ValueError("mission must be None, 'headland_first' or 'headland_last'")
    if mission is not None and not headland_paths:
        raise ValueError('mission needs headland_paths=True: the loops the mission drives')
    if patch and missed_min_area is None:
        raise ValueError('patch=True needs missed_min_area: the regions the patch passes are laid over')
    if missed_min_area is not None and coverage_resolution is None:
        raise ValueError('missed_min_area needs coverage_resolution: the grid the missed regions are found on')
    if detour and not (reshape and headland_paths):
        raise ValueError('detour=True needs reshape=True and headland_paths=True: the loops the blocked legs ride')
    if reshape and clear_of is None:
        raise ValueError('reshape=True needs clear_of: the region the connectors have to stay clear of')
    if price_clear and not reshape:
        raise ValueError('price_clear=True needs reshape=True: the route would be priced with words the field paths do not drive')
    torch = _torch()
    fields = polygon_fields(fields, device)
    lines, work = headland(fields, width, passes, arc_step=arc_step, device=device)
    ang = _dev_f64(angles, work.x.device).reshape(-1)
    idx, _ = best_swath_angle(work, ang, width, turn_cost, device=device)
    # (a field without a valid angle is cut at angles[0]: its status there is non-zero, as at every angle)
    chosen = ang[idx.clamp(min=0)] if ang.numel() else torch.zeros(work.n, dtype=torch.float64, device=work.x.device)
    ss = polygon_swaths(work, chosen, width, device=device)
    region = None if clear_of is None else (fields if isinstance(clear_of, str) and clear_of == 'boundary' else polygon_fields(clear_of, device))
    route = route_swaths(ss, radius, reversing=reversing, entry=entry, exit=exit, starts=starts, spacing=spacing, device=device, clear_of=region,
                         **({'price_clear': True} if price_clear else {}))
    hp = _drive_headland(lines, radius, spacing, reversing=reversing, device=device) if headland_paths else None
    both = (hp, _drive_headland(lines, radius, spacing, reversing=reversing, direction=-1, device=device)) if detour else None
    path_ends = {} if mission is not None else {'entry': entry, 'exit': exit}          # (a mission's gates are joined to its first and last item)
    paths = field_paths(ss, radius, spacing, reversing=reversing, order=route, device=device, clear_of=region if reshape else None,
                        **path_ends, **({'loops': both} if detour else {}))
    clr = route.clearance          # (the legs field_paths drives: route_swaths planned at the same _chord_radius(radius, spacing))
    cov = None
    if coverage_resolution is not None:
        cov = polygon_coverage(fields, width, coverage_resolution, paths=(paths,) if hp is None else (paths, hp), device=device,
                               **({} if missed_min_area is None else {'want_grid': True}))
    missed = None if missed_min_area is None else coverage_regions(cov, kind='missed', min_area=float(missed_min_area), device=device,
                                                                   **({'want_labels': True} if patch else {}))
    plan = PolygonPlan(lines, work, idx, chosen, ss, route, paths, hp, cov, clr, paths.transits if detour else None, missed)
    if patch:
        plan.patch, plan.patch_info = patch_swaths(missed, width, chosen, device=device)
        proute = route_swaths(plan.patch, radius, reversing=reversing, spacing=spacing, device=device)
        pp = plan.patch_paths = field_paths(plan.patch, radius, spacing, reversing=reversing, order=proute, device=device)
        as_set = (pp.offsets, pp.x, pp.y, torch.arange(fields.n, dtype=torch.int64, device=pp.x.device), pp.part == 0, pp.leg + (1 << 30))
        plan.coverage_after = polygon_coverage(fields, width, coverage_resolution, paths=((paths,) if hp is None else (paths, hp)) + (as_set,),
                                               want_grid=True, device=device)
    if mission is not None:
        open_sets = (paths,) if plan.patch_paths is None else (paths, plan.patch_paths)
        plan.mission = mission_paths((hp,) + open_sets if mission == 'headland_first' else open_sets + (hp,), radius, spacing, reversing=reversing,
                                     entry=entry, exit=exit, device=device, innermost_first=mission == 'headland_last', n_fields=fields.n,
                                     clear_of=region)
    if speeds is not None:
        plan.speeds = path_speeds(plan.mission if plan.mission is not None else paths, speeds, device=device)
    return plan


def _polys(polygons):
    """list of vertex lists -> (L.Polys, keep-alive arrays)"""
    offs, px, py = [0], [], []
    for poly in polygons:
        for (a, b) in poly:
            px.append(float(a))
            py.append(float(b))
        offs.append(len(px))
    o, ax, ay = np.asarray(offs, dtype=np.int64), np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64)
    return L.Polys(len(offs) - 1, o.ctypes.data_as(L.c_i64_p), ax.ctypes.data_as(L.c_double_p), ay.ctypes.data_as(L.c_double_p)), [o, ax, ay]


def validate(x, y, v, vehicle, field_polygons=None, obstacles=None, obstacle_offsets=None, geofence_tol=1e-6, offsets=None, device=None):
    """fcpp_validate: lateral-acceleration / geofence / obstacle flags and per-path statistics of caller-supplied paths.
    field_polygons: one vertex list per path (or None); obstacles: vertex lists; obstacle_offsets: n_paths + 1 indices into them (None: every
    path against all).  -> (flags uint32 tensor, dict of numpy arrays per path)"""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    x, y, v = _dev_f64(x, dev), _dev_f64(y, dev), _dev_f64(v, dev)
    off, off_h = _offsets(offsets, x.numel(), dev)
    n_paths = off.numel() - 1
    opt = make_options(geofence_tol=geofence_tol)
    fp, keep1 = _polys(field_polygons) if field_polygons is not None else (None, None)
    ob, keep2 = _polys(obstacles) if obstacles else (None, None)
    oo = np.ascontiguousarray(obstacle_offsets, dtype=np.int64) if obstacle_offsets is not None else None
    flags = torch.empty(x.numel(), dtype=torch.int32, device=dev)
    stats = torch.zeros((n_paths, L.STATS_WORDS), dtype=torch.int64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_validate(ctx.handle, C.byref(vehicle), C.byref(opt), n_paths, _ptr(off), x.numel(), _ptr(x), _ptr(y), _ptr(v),
                                  C.byref(fp) if fp is not None else None, C.byref(ob) if ob is not None else None, _host_ptr(oo), _ptr(flags),
                                  _ptr(stats), _host_ptr(off_h)))
    raw = stats.cpu().numpy()
    out = {}
    for k, (n, _) in enumerate(L.FieldStats._fields_):
        col = raw[:, k]
        out[n] = col.view(np.float64).copy() if k < L.STATS_DOUBLES else col.copy()
    return flags, out


def straight_segments(segs, n_points, device=None):
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    segs = _dev_f64(segs, dev).reshape(-1, 4)
    out = torch.empty((segs.shape[0], int(n_points), 2), dtype=torch.float64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_straight_segments(ctx.handle, segs.shape[0], _ptr(segs), int(n_points), _ptr(out)))
    return out


def corner_turns(corners, corner_index, with_reverse, vehicle, field_length, field_width, device=None):
    """Corner turns as a batch (fcpp_corner_turns; MLP:1580-1608 and 1024-1084 / 1154-1288): for every corner the 15-point
    quarter arc and, where with_reverse is set, the tangent reverse fill toward the box [0, L] x [0, H].
    -> list of (turn (15, 2), reverse (n, 2) or None) numpy arrays."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    c = _dev_f64(corners, dev).reshape(-1, 2)
    n = int(c.shape[0])
    ci = torch.as_tensor(np.ascontiguousarray(corner_index, dtype=np.int32), device=dev)
    rv = torch.as_tensor(np.ascontiguousarray(with_reverse, dtype=np.int32), device=dev)
    stride = 15 + max(10, int(3.0 * vehicle.min_turn_radius / 0.5))
    out = torch.empty((n, stride, 2), dtype=torch.float64, device=dev)
    counts = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_corner_turns(ctx.handle, C.byref(vehicle), n, _ptr(c), _ptr(ci), _ptr(rv), float(field_length),
                                      float(field_width), stride, _ptr(out), _ptr(counts)))
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    res = []
    for k in range(n):
        nt, nr = int(counts[k, 0]), int(counts[k, 1])
        res.append((out[k, :nt].copy(), out[k, nt:nt + nr].copy() if nr else None))
    return res


def fresnel(t, device=None):
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    t = _dev_f64(t, dev)
    c, s = torch.empty_like(t), torch.empty_like(t)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_fresnel(ctx.handle, t.numel(), _ptr(t), _ptr(c), _ptr(s)))
    return c, s


def ga_fitness(routes, D, order_mode=0, device=None):
    """-> (distance, fitness) tensors for a population of tours (GA:168-181)."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    D = _dev_f64(D, dev)
    n = D.shape[0]
    if isinstance(routes, torch.Tensor):
        r = routes.to(device=dev, dtype=torch.int32).contiguous()
    else:
        r = torch.as_tensor(np.ascontiguousarray(routes, dtype=np.int32), device=dev)
    r = r.reshape(-1, n)
    dist = torch.empty(r.shape[0], dtype=torch.float64, device=dev)
    fit = torch.empty_like(dist)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_ga_fitness(ctx.handle, n, r.shape[0], _ptr(D), _ptr(r), _ptr(dist), _ptr(fit),
                                    int(order_mode)))
    return dist, fit


def distance_matrix(xy, device=None):
    """Centroid distance matrix (MVP:229-259, MFP:263-288) -> (n, n) float64 device tensor; row 0 = the depot by convention."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    p = _dev_f64(xy, dev).reshape(-1, 2)
    x, y = p[:, 0].contiguous(), p[:, 1].contiguous()
    n = int(x.shape[0])
    D = torch.empty((n, n), dtype=torch.float64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_distance_matrix(ctx.handle, n, _ptr(x), _ptr(y), _ptr(D)))
    return D


def best_connections(from_lists, to_lists, device=None):
    """Shortest exit -> entry connection for a batch of node pairs (MFP:290-320).  from_lists[p] / to_lists[p]: (k, 2) candidate
    points of pair p.  -> (index into from_lists[p], index into to_lists[p], distance) as numpy arrays (-1, -1, inf for empty lists)."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    n = len(from_lists)
    f = [np.asarray(a, dtype=np.float64).reshape(-1, 2) for a in from_lists]
    t = [np.asarray(a, dtype=np.float64).reshape(-1, 2) for a in to_lists]
    fo = np.concatenate([[0], np.cumsum([len(a) for a in f])]).astype(np.int64)
    to = np.concatenate([[0], np.cumsum([len(a) for a in t])]).astype(np.int64)
    fxy = np.vstack(f) if n else np.zeros((0, 2))
    txy = np.vstack(t) if n else np.zeros((0, 2))
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    fo_d, to_d, fx, fy, tx, ty = d(fo), d(to), d(fxy[:, 0]), d(fxy[:, 1]), d(txy[:, 0]), d(txy[:, 1])
    bf = torch.empty(n, dtype=torch.int32, device=dev)
    bt = torch.empty(n, dtype=torch.int32, device=dev)
    bd = torch.empty(n, dtype=torch.float64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_best_connections(ctx.handle, n, _ptr(fo_d), _ptr(to_d), _ptr(fx), _ptr(fy), _ptr(tx), _ptr(ty), _ptr(bf), _ptr(bt),
                                          _ptr(bd)))
    bf, bt = bf.cpu().numpy().astype(np.int64), bt.cpu().numpy().astype(np.int64)
    ok = bf >= 0
    return np.where(ok, bf - fo[:-1], -1), np.where(ok, bt - to[:-1], -1), bd.cpu().numpy()


def ga_evolve(D, routes, cfg, seed=0, device=None):
    """The GA's evolution loop on the device (fcpp_ga_evolve; GA:64-115, 183-268).  cfg: an object with GAConfig's attributes.
    -> (final population tensor (pop, n) int32, best_route tensor, best_fitness_history, avg_fitness_history (numpy), L.GaResult)"""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    D = _dev_f64(D, dev)
    n = D.shape[0]
    if isinstance(routes, torch.Tensor):
        r = routes.to(device=dev, dtype=torch.int32).contiguous().clone()
    else:
        r = torch.as_tensor(np.ascontiguousarray(routes, dtype=np.int32), device=dev)
    r = r.reshape(-1, n)
    c = L.GaConfig(int(r.shape[0]), int(cfg.max_generations), float(cfg.crossover_rate), float(cfg.mutation_rate), int(cfg.elite_size),
                   int(cfg.tournament_size), int(cfg.convergence_threshold), 0, int(seed) & 0xffffffffffffffff)
    best = torch.empty(n, dtype=torch.int32, device=dev)
    hist = torch.zeros(2 * max(c.max_generations, 1), dtype=torch.float64, device=dev)
    res = L.GaResult()
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_ga_evolve(ctx.handle, n, C.byref(c), _ptr(D), _ptr(r), _ptr(best), _ptr(hist), C.byref(res)))
    h = hist.cpu().numpy()
    g = res.generations
    return r, best, h[:g].copy(), h[c.max_generations:c.max_generations + g].copy(), res


# ---- coverage rasterisation (include/fcpp.h: fcpp_cover_grid; MLP:1357-1371, 1426-1509) ------------------------------
def half_planes(vertices):
    """12 doubles (a, b, c) x 4 for a convex quadrilateral: inside <=> a*x + b*y + c >= 0 for all four edges."""
    v = [(float(x), float(y)) for x, y in vertices]
    area2 = sum(v[i][0] * v[(i + 1) % 4][1] - v[(i + 1) % 4][0] * v[i][1] for i in range(4))
    sgn = 1.0 if area2 > 0 else -1.0
    out = []
    for i in range(4):
        (x0, y0), (x1, y1) = v[i], v[(i + 1) % 4]
        a, b = -(y1 - y0) * sgn, (x1 - x0) * sgn            # inward normal (not normalised: only the sign is used)
        out += [a, b, -(a * x0 + b * y0)]
    return out


NOWHERE = [0.0, 0.0, -1.0] * 4      # half-planes nobody is inside of (an empty inner polygon)


def make_cover_job(ox, oy, res, nx, ny, radius, n_a, n_b=0, pts_first=0, grid_first=-1, shift=0.0, strict=True, outer=None,
                   inner=None):
    j = L.CoverJob()
    j.ox, j.oy, j.res, j.shift, j.radius = float(ox), float(oy), float(res), float(shift), float(radius)
    j.nx, j.ny, j.n_a, j.n_b = int(nx), int(ny), int(n_a), int(n_b)
    j.pts_first, j.grid_first = int(pts_first), int(grid_first)
    j.strict, j.region = int(bool(strict)), int(outer is not None)
    j.outer[:] = list(outer) if outer is not None else [0.0] * 12
    j.inner[:] = list(inner) if inner is not None else NOWHERE
    return j


def cover_grid(jobs, px, py, want_grid=False, device=None):
    """Run a list of L.CoverJob over the device (or host) point arrays px, py.
    -> (counts int64 tensor (n_jobs, 3), grid uint8 tensor or None); a job's grid is grid[j.grid_first : + nx*ny].view(ny, nx)."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    px, py = _dev_f64(px, dev), _dev_f64(py, dev)
    n = len(jobs)
    total = 0
    for j in jobs:                      # (updated in place: grid_first tells the caller where each job's grid starts)
        j.grid_first = total if want_grid else -1
        total += j.nx * j.ny if want_grid else 0
    arr = (L.CoverJob * max(n, 1))(*jobs)
    grid = torch.zeros(total, dtype=torch.uint8, device=dev) if want_grid else None
    counts = torch.zeros((n, 3), dtype=torch.int64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_cover_grid(ctx.handle, n, arr, px.numel(), _ptr(px), _ptr(py), _ptr(grid) if want_grid and total else None,
                                    _ptr(counts)))
    return counts, grid
