"""Host wrappers of the registration C-ABI (device tensors in, C calls out).

Cloud batches are `(pts4, seg_off)`: pts4 a float32 CUDA tensor (N, 4) = (x, y, z, intensity) and
seg_off an int32 tensor (S + 1,) of segment boundaries (host copy kept alongside)."""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class RegContext:
    """Owns the device arena of the registration kernels (ibl_reg_ctx)."""

    def __init__(self, arena_bytes=4 << 30):
        self._h = C.c_void_p()
        _lib.check(_lib.lib.ibl_reg_ctx_create(C.byref(self._h), int(arena_bytes)), "ibl_reg_ctx_create")

    def close(self):
        if self._h:
            _lib.lib.ibl_reg_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def reset(self):
        _lib.check(_lib.lib.ibl_reg_ctx_reset(self._h), "ibl_reg_ctx_reset")

    def status(self, clear=True):
        return _lib.lib.ibl_reg_ctx_status(self._h, 1 if clear else 0)

    def high_water(self):
        return _lib.lib.ibl_reg_ctx_high_water(self._h)

    def diag_get(self, name):
        """value of a diagnostic switch (include/ibloc.h lists them at ibl_reg_ctx_set_diag)"""
        v = C.c_double()
        _lib.check(_lib.lib.ibl_reg_ctx_get_diag(self._h, None if name is None else name.encode(), C.byref(v)), "ibl_reg_ctx_get_diag")
        return v.value

    def diag_set(self, name, value):
        """sets one switch for good (the library clamps the value); `diag()` is the form that puts the old value back"""
        _lib.check(_lib.lib.ibl_reg_ctx_set_diag(self._h, None if name is None else name.encode(), float(value)), "ibl_reg_ctx_set_diag")

    @contextlib.contextmanager
    def diag(self, **switches):
        """`with ctx.diag(feat_valu=1, spfh_qcap=8):` sets diagnostic switches of this context for the body and puts the former
        values back afterwards, also when the body raises.  For the thread that owns the context, between calls."""
        old = {name: self.diag_get(name) for name in switches}          # (an unknown name raises before anything is set)
        try:
            for name, value in switches.items():
                self.diag_set(name, value)
            yield self
        finally:
            for name, value in old.items():
                self.diag_set(name, value)


COMPACT_SCRATCH_BYTES = 64 << 20


def compact_scratch(device, bytes_needed=COMPACT_SCRATCH_BYTES):
    """the scratch chunk of `splice_rows` as a tensor of its own (at most COMPACT_SCRATCH_BYTES): allocated once, before anything is
    changed, by a caller that splices several buffers in a row"""
    return torch.empty((max(1, min(int(bytes_needed), COMPACT_SCRATCH_BYTES)),), dtype=torch.uint8, device=device)


def _scratch_rows(buf, n_used, scratch_bytes, scratch):
    """(rows per piece, the caller's scratch bytes as rows of `buf` or None) for `_move_rows`"""
    row_bytes = buf.element_size() * int(np.prod(buf.shape[1:], dtype=np.int64))
    if scratch is not None:
        scratch_bytes = scratch.numel()
    chunk = max(1, min(int(scratch_bytes) // max(row_bytes, 1), n_used))
    if scratch is not None:             # the caller's bytes as rows of this buffer (none if not even one row fits: allocated when needed)
        scratch = scratch[:chunk * row_bytes].view(buf.dtype).view((chunk,) + tuple(buf.shape[1:])) if scratch.numel() >= row_bytes else None
    return chunk, scratch


def _move_rows(buf, src, dst, length, chunk, scratch):
    """The rows [src, src + length) of `buf` move to [dst, dst + length), down or up.  A run that moves by at least its length is one
    copy.  A run that overlaps its destination goes in pieces, ascending when it moves down and descending when it moves up, so that
    no piece lands on rows still to be read: pieces of the shift's length, copied directly, when the shift is at least `chunk`
    rows, else of `chunk` rows through `scratch` (allocated here when None), so the number of copies follows the chunk, never a
    small shift.  No copy is between overlapping views.  Returns scratch."""
    shift = abs(src - dst)
    if shift >= length:
        buf[dst:dst + length].copy_(buf[src:src + length])
    elif shift > 0:
        direct = shift >= chunk                          # source and destination of a piece no longer than the shift are disjoint
        piece = shift if direct else chunk
        if not direct and scratch is None:
            scratch = torch.empty((chunk,) + tuple(buf.shape[1:]), dtype=buf.dtype, device=buf.device)
        starts = range(0, length, piece)
        for o in (starts if dst < src else reversed(starts)):
            c = min(piece, length - o)
            if direct:
                buf[dst + o:dst + o + c].copy_(buf[src + o:src + o + c])
            else:
                scratch[:c].copy_(buf[src + o:src + o + c])
                buf[dst + o:dst + o + c].copy_(scratch[:c])
    return scratch


def splice_rows(buf: torch.Tensor, n_used: int, edits, scratch=None, scratch_bytes=COMPACT_SCRATCH_BYTES):
    """The one way rows enter, leave or change place in a buffer with headroom (live memory): `edits` = [(begin, end, new_rows), ...],
    ascending and disjoint over the first n_used rows of `buf`; the rows [begin, end) give way to new_rows (a tensor of any number
    of rows of buf's row shape: none is a removal, begin == end an insertion, one insertion at n_used an append).  IN PLACE while
    the result fits -- a resident feature set is tens of GB and is never duplicated: the kept runs between the edits move first,
    those that move down in ascending and then those that move up in descending order (`_move_rows`: through one bounded scratch
    chunk of scratch_bytes), and the new rows are written last.  In that order no run lands on rows another run has yet to leave: a
    run that moves down lands below its own end, which lies below every later run; a run that moves up lands above its own begin,
    above every earlier run; and the later runs that move up, and every run that moves down, have left by then.  A result that does
    not fit is built once into a buffer 1.5 times as large (one copy of the kept rows).  Any device; everything is queued on the
    current stream.  scratch: a `compact_scratch` tensor to use (its size then stands for scratch_bytes) instead of allocating one
    when a run needs it.  Returns (buffer, view of its used rows)."""
    moves, fresh, at, to = [], [], 0, 0                  # (source, destination, length) of kept runs, (destination, rows) of new ones
    for b, e, rows in edits:
        assert at <= b <= e <= n_used and tuple(rows.shape[1:]) == tuple(buf.shape[1:])
        if b > at:
            moves.append((at, to, b - at))
            to += b - at
        if rows.shape[0]:
            fresh.append((to, rows))
            to += rows.shape[0]
        at = e
    if at < n_used:
        moves.append((at, to, n_used - at))
        to += n_used - at
    if to > buf.shape[0]:
        grown = torch.empty((max(to, buf.shape[0] + buf.shape[0] // 2),) + tuple(buf.shape[1:]), dtype=buf.dtype, device=buf.device)
        for src, dst, length in moves:
            grown[dst:dst + length].copy_(buf[src:src + length])
        buf = grown
    else:
        chunk, scratch = _scratch_rows(buf, n_used, scratch_bytes, scratch)
        for src, dst, length in moves:
            if dst < src:
                scratch = _move_rows(buf, src, dst, length, chunk, scratch)
        for src, dst, length in reversed(moves):
            if dst > src:
                scratch = _move_rows(buf, src, dst, length, chunk, scratch)
    for dst, rows in fresh:
        buf[dst:dst + rows.shape[0]].copy_(rows)
    return buf, buf[:to]


# An edit of a live batch is written once, on its segments: [(seg_begin, seg_end, new_begin, new_end), ...] -- ascending and disjoint;
# the segments [seg_begin, seg_end) give way to the segments [new_begin, new_end) of a batch of new clouds.  The three verbs:
def appended(n_seg, n_new):
    """the segment edit that puts n_new new segments behind the n_seg resident ones"""
    return [(n_seg, n_seg, 0, n_new)]


def removed(segments):
    """the segment edits that take the ascending `segments` out"""
    return [(s, s + 1, 0, 0) for s in segments]


def replaced(segments):
    """the segment edits that put new segment i in the place of segments[i] (ascending)"""
    return [(s, s + 1, i, i + 1) for i, s in enumerate(segments)]


def row_edits(off, seg_edits, new_off=(0,)):
    """the row edits [(begin, end, new_begin, new_end), ...] of the segment edits `seg_edits` on a batch with offsets `off`, the new
    batch's being `new_off`: row ranges of the old and of the new batch, neighbours joined, edits of nothing by nothing left out"""
    out = []
    for sb, se, snb, sne in seg_edits:
        b, e, nb, ne = int(off[sb]), int(off[se]), int(new_off[snb]), int(new_off[sne])
        if out and out[-1][1] == b:
            out[-1] = (out[-1][0], e, out[-1][2], ne)
        elif e > b or ne > nb:
            out.append((b, e, nb, ne))
    return [x for x in out if x[1] > x[0] or x[3] > x[2]]


def spliced_host(per_seg, seg_edits, new_per_seg):
    """the per-segment host array (sizes, bounding boxes) after the segment edits: rows [seg_begin, seg_end) give way to
    new_per_seg[new_begin:new_end]"""
    parts, at = [], 0
    for sb, se, nb, ne in seg_edits:
        parts += [per_seg[at:sb], new_per_seg[nb:ne]]
        at = se
    return np.ascontiguousarray(np.concatenate(parts + [per_seg[at:]]))


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _spliced_rows(buf, n_used, edits, rows, scratch):
    """`splice_rows` for row edits whose new rows are rows[new_begin:new_end] (rows = None: nothing new)"""
    rows = buf[:0] if rows is None else rows
    return splice_rows(buf, n_used, [(b, e, rows[nb:ne]) for b, e, nb, ne in edits], scratch=scratch)


class CloudBatch:
    """Packed clouds on the device."""

    def __init__(self, pts4: torch.Tensor, seg_off_host: np.ndarray):
        assert pts4.is_cuda and pts4.dtype == torch.float32 and pts4.dim() == 2 and pts4.shape[1] == 4 and pts4.is_contiguous()
        self.pts4 = pts4
        self._buf = pts4                 # backing buffer; longer than pts4 once the batch has headroom (from_numpy reserve_points, append)
        self.seg_off_host = np.ascontiguousarray(seg_off_host, dtype=np.int32)
        assert self.seg_off_host[-1] == pts4.shape[0]
        self.seg_off = torch.from_numpy(self.seg_off_host).to(pts4.device)

    @property
    def n_seg(self):
        return len(self.seg_off_host) - 1

    @property
    def n(self):
        return int(self.seg_off_host[-1])

    def as_pool(self, features=None):
        """the batch as the ibl_cloud_pool a registration call takes, with the InstanceFeatures of its clouds or none.  The struct holds
        what its pointers need alive (tensors, host arrays, the feature struct): keep IT until the call has returned."""
        pool = _PoolStruct(self.pts4.data_ptr(), self.seg_off.data_ptr(), self.seg_off_host.ctypes.data, None, self.n_seg)
        pool._keep = (self.pts4, self.seg_off, self.seg_off_host, features)
        if features is not None:
            pool._feat = features.as_struct()
            pool.features = C.addressof(pool._feat)
        return pool

    @staticmethod
    def from_numpy(clouds, intensities=None, device="cuda", reserve_points=0):
        """clouds: list of (n_i, 3) arrays; intensities: list of (n_i,) or None (zeros).  reserve_points: room for that many further
        points behind the clouds (`append` then copies only what it adds)."""
        sizes = [len(c) for c in clouds]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        p4 = np.zeros((int(off[-1]), 4), dtype=np.float32)
        for i, c in enumerate(clouds):
            p4[off[i]:off[i + 1], :3] = np.asarray(c, dtype=np.float32)
            if intensities is not None:
                p4[off[i]:off[i + 1], 3] = np.asarray(intensities[i], dtype=np.float32)
        if reserve_points <= 0:
            return CloudBatch(torch.from_numpy(p4).to(device), off)
        buf = torch.empty((len(p4) + int(reserve_points), 4), dtype=torch.float32, device=device)
        buf[:len(p4)].copy_(torch.from_numpy(p4))
        batch = CloudBatch(buf[:len(p4)], off)
        batch._buf = buf
        return batch

    def _splice(self, seg_edits, new: "CloudBatch" = None, scratch=None):
        """The one edit behind `append`, `remove` and `replace`: the segment edits `seg_edits` (above `row_edits`) with the clouds of
        `new` (None: nothing new).  The rows move in the backing buffer (`splice_rows`), the offsets follow from the sizes.  Returns
        the row edits."""
        new_off = (0,) if new is None else new.seg_off_host
        edits = row_edits(self.seg_off_host, seg_edits, new_off)
        if self.n + sum((ne - nb) - (e - b) for b, e, nb, ne in edits) > 0x7FFFFFF0:
            raise ValueError("more than 0x7FFFFFF0 points in a cloud batch")
        self._buf, self.pts4 = _spliced_rows(self._buf, self.n, edits, None if new is None else new.pts4, scratch)
        self.seg_off_host = offsets_of(spliced_host(np.diff(self.seg_off_host), seg_edits, np.diff(new_off)))
        self.seg_off = torch.from_numpy(self.seg_off_host).to(self.pts4.device)
        return edits

    def append(self, clouds, intensities=None):
        """Further clouds behind the last one (segments n_seg ..): `clouds` / `intensities` as `from_numpy` takes them, or a CloudBatch
        on the same device.  Only the new points are copied unless the buffer has to grow (by 1.5).  `pts4` and `seg_off` are NEW
        tensor objects afterwards (pts4 a longer view of the same buffer when it did not grow)."""
        new = clouds if isinstance(clouds, CloudBatch) else CloudBatch.from_numpy(clouds, intensities, device=self.pts4.device)
        self._splice(appended(self.n_seg, new.n_seg), new)
        return new

    def remove(self, segments, scratch=None):
        """Takes the clouds `segments` (ascending, distinct segment indices; not all of them) out of the batch: the later clouds move
        down in the backing buffer (`splice_rows`, in place) and take the lower segment indices.  `pts4` and `seg_off` are NEW tensor
        objects afterwards.  Returns the point ranges [(begin, end), ...] that were removed, in the numbering before the call
        (neighbouring clouds joined) -- what `MemGrid.remove` and `InstanceFeatures.remove` take.  scratch: see `splice_rows`."""
        segments = [int(s) for s in segments]
        assert all(a < b for a, b in zip([-1] + segments, segments + [self.n_seg])) and len(segments) < self.n_seg
        return [(b, e) for b, e, _, _ in self._splice(removed(segments), scratch=scratch)]

    def replace(self, segments, new_batch: "CloudBatch", scratch=None):
        """Puts cloud i of `new_batch` (a CloudBatch on the same device with len(segments) clouds) in the place of the cloud
        segments[i] (ascending, distinct segment indices): every cloud keeps its segment index, the clouds behind a replaced one move
        in the backing buffer (`splice_rows`: in place unless it has to grow by 1.5).  `pts4` and `seg_off` are NEW tensor objects
        afterwards.  Returns the edits [(begin, end, new_begin, new_end), ...] (`row_edits`: point ranges in the numbering
        before the call and the rows of new_batch that took their place) -- what `InstanceFeatures.replace` takes."""
        segments = [int(s) for s in segments]
        assert all(a < b for a, b in zip([-1] + segments, segments + [self.n_seg])) and new_batch.n_seg == len(segments)
        return self._splice(replaced(segments), new_batch, scratch=scratch)


def unproject_masks(ctx: RegContext, depth: torch.Tensor, rgb: torch.Tensor, masks: torch.Tensor, fx: float, fy: float,
                    depth_factor: float = 1.0, want_f64: bool = False):
    """One coloured cloud per instance mask from a depth image (get_mask_coloured_pointclouds_from_depth,
    utils/depth_utils.py:176-206, before its outlier step).  depth (H, W) float32, float64 or uint16 (int16 storage is read as uint16), rgb (H, W, 3)
    uint8, masks (n, H, W) bool / uint8 -- device tensors.  Returns the clouds as a CloudBatch (x, y, z, intensity); with want_f64 also
    (points, colours) as (N, 3) float64 device tensors holding exactly the values of the reference's Open3D clouds (memory build)."""
    dev = depth.device
    assert depth.is_cuda and rgb.is_cuda and masks.is_cuda and depth.dim() == 2
    H, W = depth.shape
    if depth.dtype in (torch.uint16, torch.int16):         # int16 storage = the bits of a uint16 image
        is_u16, d = 1, depth.contiguous()
    elif depth.dtype == torch.float32:
        is_u16, d = 0, depth.contiguous()                  # numpy keeps float32 arithmetic for a float32 depth image
    else:
        is_u16, d = 2, depth.to(torch.float64).contiguous()
    rgb = rgb.to(torch.uint8).contiguous()
    m = masks.reshape(-1, H, W).to(torch.uint8).contiguous()
    n = m.shape[0]
    assert rgb.shape == (H, W, 3)
    cap = int(m.count_nonzero().item()) if n else 0           # a mask pixel yields at most one point
    pts4 = torch.empty((max(cap, 1), 4), dtype=torch.float32, device=dev)
    off_dev = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    off_host = np.zeros(n + 1, dtype=np.int32)
    p64 = torch.empty((max(cap, 1), 3), dtype=torch.float64, device=dev) if want_f64 else None
    c64 = torch.empty((max(cap, 1), 3), dtype=torch.float64, device=dev) if want_f64 else None
    st = _lib.lib.ibl_unproject_masks(ctx.handle, d.data_ptr(), is_u16, rgb.data_ptr(), m.data_ptr(), n, H, W, float(fx), float(fy),
                                      float(depth_factor), pts4.data_ptr(), p64.data_ptr() if want_f64 else None,
                                      c64.data_ptr() if want_f64 else None, cap, off_dev.data_ptr(), off_host.ctypes.data, _stream())
    _lib.check(st, "ibl_unproject_masks")
    batch = CloudBatch(pts4[:int(off_host[-1])].contiguous() if off_host[-1] != cap or cap == 0 else pts4, off_host)
    if want_f64:
        return batch, p64[:int(off_host[-1])], c64[:int(off_host[-1])]
    return batch


def radius_outlier_batch(ctx: RegContext, batch: CloudBatch, radius: float, nb_points: int) -> torch.Tensor:
    keep = torch.empty(max(batch.n, 1), dtype=torch.uint8, device=batch.pts4.device)
    st = _lib.lib.ibl_radius_outlier_batch(ctx.handle, batch.pts4.data_ptr(), batch.seg_off.data_ptr(),
                                           batch.seg_off_host.ctypes.data, batch.n_seg, float(radius), int(nb_points),
                                           keep.data_ptr(), _stream())
    _lib.check(st, "ibl_radius_outlier_batch")
    return keep[:batch.n]


def normals_fpfh_batch(ctx: RegContext, batch: CloudBatch, radius_normal, max_nn_normal=30, radius_feature=None,
                       max_nn_feature=100):
    dev = batch.pts4.device
    normals = torch.empty((max(batch.n, 1), 4), dtype=torch.float32, device=dev)
    fpfh = torch.empty((max(batch.n, 1), 33), dtype=torch.float32, device=dev) if radius_feature else None
    st = _lib.lib.ibl_normals_fpfh_batch(ctx.handle, batch.pts4.data_ptr(), batch.seg_off.data_ptr(),
                                         batch.seg_off_host.ctypes.data, batch.n_seg, float(radius_normal), int(max_nn_normal),
                                         float(radius_feature or 0.0), int(max_nn_feature), normals.data_ptr(),
                                         fpfh.data_ptr() if fpfh is not None else None, _stream())
    _lib.check(st, "ibl_normals_fpfh_batch")
    return normals[:batch.n], (fpfh[:batch.n] if fpfh is not None else None)


# "matching order" of the 33 FPFH bins (histogram centres outwards, interleaved): instance features store their rows in this
# order, the feature search sums its squared differences in it (csrc/reg_fpfh.hip FEAT_POS, oracle/oracle_reg.c FEAT_ORDER)
FEAT_ORDER = np.array([b * 11 + c for c in (5, 4, 6, 3, 7, 2, 8, 1, 9, 0, 10) for b in (1, 2, 0)], dtype=np.int64)
# the constant the fp16 search operands are centred by (csrc/reg_common.h FM_MU; matching order)
FEAT_MU = np.array([87, 46, 101, 26, 28, 17, 26, 26, 17, 14, 21, 7, 14, 19, 7, 8, 14, 6, 8, 13, 6, 5, 11, 6, 5, 10, 6, 3, 7, 14, 3, 6, 14],
                   dtype=np.float32)


class _FeatStruct(C.Structure):
    _fields_ = [("normals4", C.c_void_p), ("fpfh", C.c_void_p), ("fpfh_split", C.c_void_p), ("fpfh_norm", C.c_void_p),
                ("grad4", C.c_void_p), ("bbox", C.c_void_p),
                ("voxel_size", C.c_double), ("grad_radius", C.c_double)]


class _PoolStruct(C.Structure):              # ibl_cloud_pool
    _fields_ = [("pts4", C.c_void_p), ("off_dev", C.c_void_p), ("off_host", C.c_void_p), ("features", C.c_void_p), ("n_seg", C.c_int32)]


class _ParamsStruct(C.Structure):            # ibl_register_params
    _fields_ = [("voxel_size", C.c_double), ("global_dist_factor", C.c_double), ("local_dist_factor", C.c_double), ("seed", C.c_uint64),
                ("ransac_max_iter", C.c_int64), ("job_id_base", C.c_uint32), ("flags", C.c_int32)]


class _OutStruct(C.Structure):               # ibl_register_out
    _fields_ = [("T", C.c_void_p), ("rmse", C.c_void_p), ("fitness", C.c_void_p), ("means", C.c_void_p), ("T_ransac", C.c_void_p),
                ("ransac_stats", C.c_void_p), ("reuse_stats", C.c_void_p)]


class InstanceFeatures:
    """Registration features of every cloud of a batch, resident on the device (ibl_instance_features): normals,
    FPFH and (for memory instances) colour gradients, plus host bounding boxes.  fpfh_split is None for COMPACT features (168 instead
    of 264 bytes per point): the feature search then builds its fp16 operands from the fp32 rows while it stages them."""

    DEVICE_ARRAYS = ("normals", "fpfh", "fpfh_split", "fpfh_norm", "grad")

    def __init__(self, normals, fpfh, fpfh_split, fpfh_norm, grad, bbox, voxel_size, grad_radius, n=None, n_seg=None):
        self.normals, self.fpfh, self.grad, self.bbox = normals, fpfh, grad, bbox
        self.fpfh_split, self.fpfh_norm = fpfh_split, fpfh_norm
        self.voxel_size, self.grad_radius = float(voxel_size), float(grad_radius)
        self.n, self.n_seg = n, n_seg          # points / clouds described (instance_features_batch sets them; `append` needs them)
        self._bufs = {}                        # backing buffers of arrays that are views with headroom behind them

    def _splice(self, verb, seg_edits, edits, new: "InstanceFeatures" = None, scratch=None):
        """The one edit behind `append`, `remove` and `replace`: the segment edits `seg_edits` and their row edits `edits` (those of
        the clouds' batch) with the features `new` (None: nothing new).  Every device array that is present is spliced in its backing
        buffer (`splice_rows`), the bounding-box rows of the clouds follow the segments."""
        if self.n is None or (new is not None and new.n is None):
            raise ValueError(f"InstanceFeatures.{verb}: point counts unknown (features not made by instance_features_batch)")
        if new is not None:
            if (self.voxel_size, self.grad_radius) != (new.voxel_size, new.grad_radius):
                raise ValueError(f"InstanceFeatures.{verb}: the features were computed with other parameters")
            for name in self.DEVICE_ARRAYS:
                if (getattr(self, name) is None) != (getattr(new, name) is None):
                    raise ValueError(f"InstanceFeatures.{verb}: `{name}` is present on one side only")
            if new.n_seg != sum(ne - nb for _, _, nb, ne in seg_edits):
                raise ValueError(f"InstanceFeatures.{verb}: as many new clouds as segments")
        for name in self.DEVICE_ARRAYS:
            cur = getattr(self, name)
            if cur is not None:
                self._bufs[name], view = _spliced_rows(self._bufs.get(name, cur), self.n, edits, None if new is None else getattr(new, name), scratch)
                setattr(self, name, view)
        self.bbox = spliced_host(self.bbox[:self.n_seg], seg_edits, self.bbox[:0] if new is None else new.bbox[:new.n_seg])
        self.n += sum((ne - nb) - (e - b) for b, e, nb, ne in edits)
        self.n_seg = len(self.bbox)

    def append(self, new: "InstanceFeatures"):
        """Attaches the features of further clouds (computed on their own: a feature depends on its own cloud only, DESIGN (c)
        conventions 5 and 7) behind the resident ones.  Same parameters and same form (compact or not, with gradients or not) only.
        The arrays are views of buffers with headroom; only the new rows are copied unless a buffer has to grow (by 1.5)."""
        self._splice("append", appended(self.n_seg, new.n_seg), [(self.n, self.n, 0, new.n)], new)

    def remove(self, segments, point_ranges, scratch=None):
        """Takes the features of the clouds `segments` (ascending, distinct) out: `point_ranges` are the point ranges of those clouds
        as `CloudBatch.remove` returns them.  Every device array that is present is compacted in its backing buffer
        (`splice_rows`: in place, nothing is duplicated or recomputed -- a feature depends on its own cloud only), the bounding-box
        rows of the clouds are dropped.  scratch: see `splice_rows`."""
        self._splice("remove", removed(list(segments)), [(b, e, 0, 0) for b, e in point_ranges], scratch=scratch)

    def replace(self, segments, point_ranges, new: "InstanceFeatures", scratch=None):
        """Puts the features `new` of len(segments) clouds (computed on their own, as for `append`) in the place of those of the
        clouds `segments` (ascending, distinct): `point_ranges` are the edits `CloudBatch.replace` returns.  Same parameters and same
        form only, as `append`.  Every device array that is present is spliced in its backing buffer (`splice_rows`: in place
        unless it has to grow, nothing resident is recomputed), the bounding-box rows of the clouds are replaced."""
        self._splice("replace", replaced(list(segments)), point_ranges, new, scratch=scratch)

    def as_struct(self):
        return _FeatStruct(self.normals.data_ptr(), self.fpfh.data_ptr(), self.fpfh_split.data_ptr() if self.fpfh_split is not None else None,
                           self.fpfh_norm.data_ptr(),
                           self.grad.data_ptr() if self.grad is not None else None,
                           self.bbox.ctypes.data, self.voxel_size, self.grad_radius)


def instance_features_batch(ctx: RegContext, batch: CloudBatch, voxel_size: float, grad_radius: float = 0.0,
                            compact: bool = False, reserve_points: int = 0) -> InstanceFeatures:
    """Normals (2 voxel, 30 nn), FPFH (5 voxel, 100 nn) and, with grad_radius > 0, colour gradients (grad_radius, 30 nn) of
    every cloud on its own, in the frame it is stored in -- what ibl_register_jobs reuses across jobs.
    compact: do not keep the rows a second time as fp16 search operands (96 of the 264 bytes per point; same registration results,
    the matrix-core search converts on the fly -- for memories whose resident features would not fit otherwise).
    reserve_points: the arrays are allocated with room for that many further points (InstanceFeatures.append) and exposed as views."""
    dev = batch.pts4.device
    n = max(batch.n, 1) + max(int(reserve_points), 0)
    normals = torch.empty((n, 4), dtype=torch.float32, device=dev)
    fpfh = torch.empty((n, 33), dtype=torch.float32, device=dev)
    # the rows once more as fp16 search operands (csrc/reg_featnn.hip)
    fpfh_split = None if compact else torch.empty((n, 48), dtype=torch.float16, device=dev)
    fpfh_norm = torch.empty((n,), dtype=torch.float32, device=dev)
    grad = torch.empty((n, 4), dtype=torch.float32, device=dev) if grad_radius > 0 else None
    bbox = np.zeros((max(batch.n_seg, 1), 6), dtype=np.float32)
    st = _lib.lib.ibl_instance_features_batch(ctx.handle, batch.pts4.data_ptr(), batch.seg_off.data_ptr(), batch.seg_off_host.ctypes.data,
                                              batch.n_seg, float(voxel_size), float(grad_radius), normals.data_ptr(), fpfh.data_ptr(),
                                              fpfh_split.data_ptr() if fpfh_split is not None else None, fpfh_norm.data_ptr(),
                                              grad.data_ptr() if grad is not None else None, bbox.ctypes.data, _stream())
    _lib.check(st, "ibl_instance_features_batch")
    feat = InstanceFeatures(normals, fpfh, fpfh_split, fpfh_norm, grad, bbox, voxel_size, grad_radius, n=batch.n, n_seg=batch.n_seg)
    if reserve_points > 0:
        for name in InstanceFeatures.DEVICE_ARRAYS:
            if getattr(feat, name) is not None:
                feat._bufs[name] = getattr(feat, name)
                setattr(feat, name, feat._bufs[name][:batch.n])
    return feat


REG_HAVE_COLORS = 1
REG_CENTER = 2
REG_FIXED_BUDGET = 4        # benchmark only: RANSAC walks exactly ransac_max_iter hypotheses per job (no confidence exit)


def _register_args(J, voxel_size, global_dist_factor, local_dist_factor, seed, job_id_base, ransac_max_iter, have_colors, center, fixed_budget):
    """params struct, out struct and the dict of host arrays (room for J jobs) the out struct points into"""
    flags = (REG_HAVE_COLORS if have_colors else 0) | (REG_CENTER if center else 0) | (REG_FIXED_BUDGET if fixed_budget else 0)
    params = _ParamsStruct(float(voxel_size), float(global_dist_factor), float(local_dist_factor), int(seed), int(ransac_max_iter),
                           int(job_id_base), flags)
    res = dict(T=np.zeros((J, 16)), rmse=np.zeros(J), fitness=np.zeros(J), means=np.zeros((J, 2, 3)), T_ransac=np.zeros((J, 16)),
               ransac_stats=np.zeros((J, 3), dtype=np.int64), reuse=np.zeros(6, dtype=np.int64))
    out = _OutStruct(*(res[k].ctypes.data for k in ("T", "rmse", "fitness", "means", "T_ransac", "ransac_stats", "reuse")))
    return params, out, res


def _job_results(res, J):
    """the first J jobs of the host arrays of _register_args as the wrappers return them"""
    r = {k: (v if k == "reuse" else v[:J]) for k, v in res.items()}
    r["T"], r["T_ransac"] = r["T"].reshape(J, 4, 4), r["T_ransac"].reshape(J, 4, 4)
    return r


def register_batch(ctx: RegContext, det: CloudBatch, mem: CloudBatch, job_src_seg, job_tgt_seg, voxel_size,
                   global_dist_factor=1.5, local_dist_factor=0.4, seed=0, job_id_base=0, ransac_max_iter=4000000,
                   have_colors=True, center=True, det_features: InstanceFeatures = None, mem_features: InstanceFeatures = None,
                   job_ids=None, fixed_budget=False):
    """Batched register_point_clouds (utils/fpfh_register.py:100-143).  job_*_seg: (J, <=3) int arrays of
    pool segment ids (-1 padded).  det_features / mem_features: instance features of the two pools
    (instance_features_batch); the results do not depend on them, only the work does.  Returns dict of host arrays:
    T (J,4,4), rmse, fitness, means (J,2,3), T_ransac (J,4,4), ransac_stats (J,3), reuse (points served by the instance
    features, points recomputed, recomputed groups, job sides, distinct matching pairs, pair uses).
    job_ids: (J,) explicit RANSAC ids instead of job_id_base + j (jobs routed between ranks keep theirs)."""
    def pad(a):
        a = np.asarray(a, dtype=np.int32)
        if a.ndim == 1:
            a = a[:, None]
        out = np.full((a.shape[0], 3), -1, dtype=np.int32)
        out[:, :a.shape[1]] = a
        return np.ascontiguousarray(out)

    js, jt = pad(job_src_seg), pad(job_tgt_seg)
    J = js.shape[0]
    assert jt.shape[0] == J
    ids = None if job_ids is None else np.ascontiguousarray(job_ids, dtype=np.uint32)
    assert ids is None or ids.shape == (J,)
    params, out, res = _register_args(J, voxel_size, global_dist_factor, local_dist_factor, seed, job_id_base, ransac_max_iter, have_colors,
                                      center, fixed_budget)
    det_pool, mem_pool = det.as_pool(det_features), mem.as_pool(mem_features)
    st = _lib.lib.ibl_register_jobs(ctx.handle, C.byref(det_pool), C.byref(mem_pool), js.ctypes.data, jt.ctypes.data,
                                    None if ids is None else ids.ctypes.data, J, C.byref(params), C.byref(out), _stream())
    _lib.check(st, "ibl_register_jobs")
    return _job_results(res, J)


def register_evaluate_batch(ctx: RegContext, det: CloudBatch, q_per_frame, assns, mem: CloudBatch, mem_features: InstanceFeatures, grid,
                            voxel_size, global_dist_factor, local_dist_factor, outlier_radius=0.05, outlier_nb_points=8, eval_threshold=0.02,
                            seed=0, job_id_base=0, ransac_max_iter=4000000, have_colors=True, center=True, fixed_budget=False):
    """Stage B of localise() in one library call (`ibl_register_evaluate_batch`, csrc/localise.hip): outlier removal + compaction, the
    detections' features, registration of every candidate assignment, whole-memory evaluation, winner per frame.  assns: per frame the
    list of assignments [[det, mem], ...] (what the assignment search returns).  Returns a dict of host arrays: clean_off (S + 1), T, rmse,
    fitness, means, T_ransac, ransac_stats, reuse, T_global, full_rmse, full_fitness (per job, frames in order) and best (per frame)."""
    q = np.ascontiguousarray(q_per_frame, dtype=np.int32)
    F = len(q)
    max_assn = max(6, max((len(a) for a in assns), default=0))
    assn = np.full((F, max_assn, 6), -1, dtype=np.int32)
    alen = np.zeros((F, max_assn), dtype=np.int32)
    acnt = np.zeros(F, dtype=np.int32)
    for f, lst in enumerate(assns):
        acnt[f] = len(lst)
        for a, pairs in enumerate(lst):
            alen[f, a] = len(pairs)
            for t, (d, m) in enumerate(pairs):
                assn[f, a, 2 * t], assn[f, a, 2 * t + 1] = d, m
    J = int(acnt.sum())
    Jc = max(J, 1)
    clean_off = np.zeros(det.n_seg + 1, dtype=np.int32)
    n_jobs = C.c_int32(0)
    params, out, res = _register_args(Jc, voxel_size, global_dist_factor, local_dist_factor, seed, job_id_base, ransac_max_iter, have_colors,
                                      center, fixed_budget)
    G = np.zeros((Jc, 16)); frmse = np.zeros(Jc); ffit = np.zeros(Jc); best = np.full(max(F, 1), -1, dtype=np.int32)
    det_pool, mem_pool = det.as_pool(), mem.as_pool(mem_features)
    st = _lib.lib.ibl_register_evaluate_batch(
        ctx.handle, C.byref(det_pool), q.ctypes.data, F, assn.ctypes.data, alen.ctypes.data, acnt.ctypes.data, max_assn, C.byref(mem_pool),
        grid.handle, C.byref(params), float(outlier_radius), int(outlier_nb_points), float(eval_threshold), Jc, clean_off.ctypes.data,
        C.byref(n_jobs), C.byref(out), G.ctypes.data, frmse.ctypes.data, ffit.ctypes.data, best.ctypes.data, _stream())
    _lib.check(st, "ibl_register_evaluate_batch")
    assert n_jobs.value == J
    return dict(_job_results(res, J), clean_off=clean_off, T_global=G[:J].reshape(J, 4, 4), full_rmse=frmse[:J], full_fitness=ffit[:J],
                best=best[:F])


class MemGrid:
    """Spatial hash over all memory points.  It owns its device memory: `close` frees it, and nothing of it lives in the context
    arena (RegContext.reset leaves it valid).  Built once and immutable unless live=True: then the grid has room for reserve_points
    further points, `append` merges further points into it, `remove` takes points out and `replace` changes points in place."""

    def __init__(self, ctx: RegContext, mem_pts4: torch.Tensor, cell=0.04, live=False, reserve_points=0):
        assert mem_pts4.is_cuda and mem_pts4.dtype == torch.float32 and mem_pts4.shape[1] == 4 and mem_pts4.is_contiguous()
        self.ctx = ctx
        self.cell = cell
        self.live = bool(live)
        self.device = mem_pts4.device
        self._h = C.c_void_p()
        st = _lib.lib.ibl_memgrid_build(ctx.handle, mem_pts4.data_ptr(), mem_pts4.shape[0], float(cell), int(self.live),
                                        int(reserve_points) if self.live else 0, C.byref(self._h), _stream())
        _lib.check(st, "ibl_memgrid_build")

    def append(self, pts4_new: torch.Tensor):
        """Merges further points (they count as the points behind all earlier ones) into a live grid: afterwards it equals the grid
        built from all points at once.  The call synchronises the current stream; no evaluation that uses the grid may be in flight
        on another stream meanwhile.  On a grid built without live=True the library refuses (IblError) and the grid is unchanged."""
        assert pts4_new.is_cuda and pts4_new.dtype == torch.float32 and pts4_new.dim() == 2 and pts4_new.shape[1] == 4 and pts4_new.is_contiguous()
        st = _lib.lib.ibl_memgrid_append(self.ctx.handle, self._h, pts4_new.data_ptr(), pts4_new.shape[0], _stream())
        _lib.check(st, "ibl_memgrid_append")

    def remove(self, ranges):
        """Takes the points whose original indices (position in the array the grid was built from, plus everything appended since) lie
        in the half-open `ranges` = [(begin, end), ...] -- ascending, disjoint, non-empty, not everything -- out of a live grid:
        afterwards it equals the grid built from the kept points, which count as renumbered from 0.  Synchronises the current stream;
        the rule for other streams is `append`'s.  Whatever the library refuses (IblError) leaves the grid unchanged."""
        rb = np.ascontiguousarray([r[0] for r in ranges], dtype=np.int64)
        re = np.ascontiguousarray([r[1] for r in ranges], dtype=np.int64)
        st = _lib.lib.ibl_memgrid_remove(self.ctx.handle, self._h, rb.ctypes.data, re.ctypes.data, len(rb), _stream())
        _lib.check(st, "ibl_memgrid_remove")

    def replace(self, ranges, counts, pts4_new: torch.Tensor):
        """Replaces the points whose original indices lie in ranges[r] = (begin, end) -- ascending, disjoint, no two with the same
        begin; an empty range is an insertion in front of `begin` -- by the next counts[r] rows of pts4_new (0: a removal) in a live
        grid: afterwards it equals the grid built from the spliced points (ibl_memgrid_replace).  Synchronises the current stream;
        the rule for other streams is `append`'s.  Whatever the library refuses (IblError) leaves the grid unchanged."""
        assert pts4_new.is_cuda and pts4_new.dtype == torch.float32 and pts4_new.dim() == 2 and pts4_new.shape[1] == 4 and pts4_new.is_contiguous()
        rb = np.ascontiguousarray([r[0] for r in ranges], dtype=np.int64)
        re = np.ascontiguousarray([r[1] for r in ranges], dtype=np.int64)
        nc = np.ascontiguousarray(counts, dtype=np.int64)
        if len(nc) != len(rb) or int(nc.sum()) != pts4_new.shape[0]:
            raise ValueError("MemGrid.replace: one count per range, and as many new rows as the counts say")
        st = _lib.lib.ibl_memgrid_replace(self.ctx.handle, self._h, rb.ctypes.data, re.ctypes.data, nc.ctypes.data,
                                          pts4_new.data_ptr() if pts4_new.shape[0] else None, len(rb), _stream())
        _lib.check(st, "ibl_memgrid_replace")

    def overlap(self, det_pts4: torch.Tensor, det_off_host, inst_off: torch.Tensor, radius, k=8, inst_off_end=None):
        """Which instances does each detection cloud overlap (ibl_memgrid_overlap; live grids only): det_pts4 the world-frame points of
        all detections (float32 (N, 4) on the device), det_off_host their n_det + 1 offsets, inst_off an int32 DEVICE tensor of
        n_inst + 1 instance offsets over the grid's original point indices (a memory's `clouds.seg_off`).  hits(d, m) = the points of
        detection d with some point of instance m at squared fp32 distance < (float)(radius * radius).  Returns numpy arrays
        (inst (n_det, k) int32, -1 padded; hits (n_det, k) int32, 0 padded; n_hit_inst (n_det,) int32): per detection the instances
        with hits > 0 by hits descending, then index ascending, cut to k, and their uncut number.  inst_off_end: the last entry of
        inst_off where the caller holds it on the host (the library checks it against the grid's point count); None reads it from
        the device.  Synchronises the current stream.  Whatever the library refuses raises IblError before anything is launched."""
        assert det_pts4.is_cuda and det_pts4.dtype == torch.float32 and det_pts4.dim() == 2 and det_pts4.shape[1] == 4 and det_pts4.is_contiguous()
        assert inst_off.is_cuda and inst_off.dtype == torch.int32 and inst_off.dim() == 1 and inst_off.is_contiguous() and len(inst_off) >= 2
        off = np.ascontiguousarray(det_off_host, dtype=np.int32)
        if len(off) < 1 or (len(off) > 1 and int(off.max()) > det_pts4.shape[0]):
            raise ValueError("MemGrid.overlap: n_det + 1 detection offsets within the rows of det_pts4 expected")
        n_det, n_inst, k = len(off) - 1, len(inst_off) - 1, int(k)
        inst = np.full((n_det, max(k, 1)), -1, dtype=np.int32)          # (k < 1 is the library's to refuse)
        hits = np.zeros((n_det, max(k, 1)), dtype=np.int32)
        n_hit = np.zeros(n_det, dtype=np.int32)
        end = int(inst_off[-1].item()) if inst_off_end is None else int(inst_off_end)
        st = _lib.lib.ibl_memgrid_overlap(self.ctx.handle, self._h, inst_off.data_ptr(), n_inst, end, det_pts4.data_ptr(),
                                          off.ctypes.data, n_det, float(radius), k, inst.ctypes.data, hits.ctypes.data, n_hit.ctypes.data,
                                          _stream())
        _lib.check(st, "ibl_memgrid_overlap")
        return inst, hits, n_hit

    def export(self):
        """copies of the grid's arrays as device tensors: dict(sorted (n, 4) float32 -- the points in cell order --, ukeys (n_cells,)
        int64 holding the unsigned 64-bit cell keys, ustart (n_cells + 1,) int32)"""
        i = self.info()
        dev = self.device
        out = dict(sorted=torch.empty((i["n"], 4), dtype=torch.float32, device=dev),
                   ukeys=torch.empty((i["n_cells"],), dtype=torch.int64, device=dev),
                   ustart=torch.empty((i["n_cells"] + 1,), dtype=torch.int32, device=dev))
        st = _lib.lib.ibl_memgrid_export(self._h, out["sorted"].data_ptr(), out["ukeys"].data_ptr(), out["ustart"].data_ptr(), _stream())
        _lib.check(st, "ibl_memgrid_export")
        return out

    def info(self):
        """dict(n, n_cells, table_slots, point_capacity, ustart_end = ustart[n_cells]) of the grid as it stands"""
        n, cap, slots = C.c_int64(), C.c_int64(), C.c_int64()
        cells, end = C.c_int32(), C.c_int32()
        st = _lib.lib.ibl_memgrid_info(self._h, C.byref(n), C.byref(cells), C.byref(slots), C.byref(cap), C.byref(end), _stream())
        _lib.check(st, "ibl_memgrid_info")
        return dict(n=n.value, n_cells=cells.value, table_slots=slots.value, point_capacity=cap.value, ustart_end=end.value)

    def close(self):
        """Frees the grid, device arrays included."""
        if self._h:
            _lib.lib.ibl_memgrid_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h


def evaluate_batch(ctx: RegContext, grid: MemGrid, det_pts4: torch.Tensor, job_begin, job_end, T_global, threshold=0.02):
    """evaluate_transform (utils/fpfh_register.py:145-150) for J candidates; returns (rmse (J,), fitness (J,))."""
    jb = np.ascontiguousarray(job_begin, dtype=np.int32)
    je = np.ascontiguousarray(job_end, dtype=np.int32)
    T = np.ascontiguousarray(T_global, dtype=np.float64).reshape(-1, 16)
    J = len(jb)
    rmse = np.zeros(J, dtype=np.float64)
    fit = np.zeros(J, dtype=np.float64)
    st = _lib.lib.ibl_evaluate_batch(ctx.handle, grid.handle, det_pts4.data_ptr(), jb.ctypes.data, je.ctypes.data, T.ctypes.data,
                                     J, float(threshold), None, rmse.ctypes.data, fit.ctypes.data, _stream())
    _lib.check(st, "ibl_evaluate_batch")
    return rmse, fit


def evaluate_points(ctx: RegContext, grid: MemGrid, det_pts4: torch.Tensor, job_begin, job_end, T_global, threshold=0.02):
    """Per-point form of `evaluate_batch`: squared distance of every transformed detected point to its nearest point of THIS grid within
    `threshold` (+inf when none) as one float32 device tensor (jobs back to back), plus this grid's own (rmse, fitness)."""
    jb = np.ascontiguousarray(job_begin, dtype=np.int32)
    je = np.ascontiguousarray(job_end, dtype=np.int32)
    T = np.ascontiguousarray(T_global, dtype=np.float64).reshape(-1, 16)
    J = len(jb)
    d2 = torch.empty(max(int((je - jb).sum()), 1), dtype=torch.float32, device=det_pts4.device)
    rmse = np.zeros(J, dtype=np.float64)
    fit = np.zeros(J, dtype=np.float64)
    st = _lib.lib.ibl_evaluate_batch(ctx.handle, grid.handle, det_pts4.data_ptr(), jb.ctypes.data, je.ctypes.data, T.ctypes.data,
                                     J, float(threshold), d2.data_ptr(), rmse.ctypes.data, fit.ctypes.data, _stream())
    _lib.check(st, "ibl_evaluate_batch")
    return d2[:int((je - jb).sum())], rmse, fit


def evaluate_information(ctx: RegContext, grid: MemGrid, det_pts4: torch.Tensor, job_begin, job_end, T_global, threshold=0.02, about=None,
                         points=False):
    """Open3D's get_information_matrix_from_point_clouds for J poses against the whole memory (`ibl_evaluate_information`): the 6 x 6
    matrix sum G^T G, G = [-[m]x | I], over the correspondences of `evaluate_batch` -- every detected point of the job whose nearest
    memory point m lies within `threshold`; among memory points at the same fp32 distance the lexicographically smallest (x, y, z).
    Rotation first, then translation; it belongs to the LEFT perturbation T' = exp(xi^) T_global, xi = (omega, v).  about: 3 doubles
    subtracted from m (None: the origin, Open3D's convention).  Returns (info (J, 6, 6) float64, n_corr (J,) int64) and, with
    points=True, the (N, 4) float32 device tensor of the matched x, y, z and d2 per point (jobs back to back; (0, 0, 0, +inf) when
    none).  n_corr / (job_end - job_begin) is `evaluate_batch`'s fitness exactly."""
    jb = np.ascontiguousarray(job_begin, dtype=np.int32)
    je = np.ascontiguousarray(job_end, dtype=np.int32)
    T = np.ascontiguousarray(T_global, dtype=np.float64).reshape(-1, 16)
    J = len(jb)
    assert len(je) == J and len(T) == J
    assert det_pts4.is_cuda and det_pts4.dtype == torch.float32 and det_pts4.dim() == 2 and det_pts4.shape[1] == 4 and det_pts4.is_contiguous()
    if J and int(je.max()) > det_pts4.shape[0]:
        raise ValueError("evaluate_information: a job ends behind the rows of det_pts4")
    ab = None if about is None else np.ascontiguousarray(about, dtype=np.float64).reshape(3)
    total = int((je.astype(np.int64) - jb).sum()) if J else 0
    nn = torch.empty((max(total, 1), 4), dtype=torch.float32, device=det_pts4.device) if points else None
    info = np.zeros((J, 6, 6), dtype=np.float64)
    n_corr = np.zeros(J, dtype=np.int64)
    st = _lib.lib.ibl_evaluate_information(ctx.handle, grid.handle, det_pts4.data_ptr(), jb.ctypes.data, je.ctypes.data, T.ctypes.data, J,
                                           float(threshold), None if ab is None else ab.ctypes.data, None if nn is None else nn.data_ptr(),
                                           info.ctypes.data, n_corr.ctypes.data, _stream())
    _lib.check(st, "ibl_evaluate_information")
    return (info, n_corr, nn[:max(total, 0)]) if points else (info, n_corr)
