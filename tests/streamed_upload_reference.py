"""What the streamed upload (include/ceres_hip.h: ceres_hip_values_begin / _ready / _end) must do, restated in plain numpy and
independently of the C loop in csrc/plan.cc (PlanValueStreams): which bytes a run of row blocks owns, how many value streams a layout
has, and what the device must hold once _end has returned.  Nothing here imports the package's native code.

A cell is (row block r, column block j, position p): it owns the doubles [p, p + row_block_size[r] * col_block_size[j]) of the value
array.  Class 0 of a row is its first cell, class 1 its other cells."""
import numpy as np


def cells(bs):
    """(row block, start, end, class, column block) of every cell, in row order."""
    ptr = bs.row_cell_ptr.astype(np.int64)
    row = np.repeat(np.arange(bs.num_row_blocks, dtype=np.int64), np.diff(ptr))
    col = bs.cell_col_block.astype(np.int64)
    start = bs.cell_value_pos.astype(np.int64)
    end = start + bs.row_block_size.astype(np.int64)[row] * bs.col_block_size.astype(np.int64)[col]
    cls = (np.arange(col.shape[0]) != ptr[row]).astype(np.int64)
    return row, start, end, cls, col


def _one_run(start, end):
    """Do these cells, in this order, lie back to back?  (No cell: yes.)"""
    return bool(start.shape[0] == 0 or np.array_equal(start[1:], end[:-1]))


def value_streams(bs):
    """1 if all cells, in row order, lie back to back in one run; else 2 if the rows' first cells do and their other cells do; else 0."""
    _, start, end, cls, _ = cells(bs)
    if _one_run(start, end):
        return 1
    if _one_run(start[cls == 0], end[cls == 0]) and _one_run(start[cls == 1], end[cls == 1]):
        return 2
    return 0


def run_bytes(bs, r0, r1):
    """(value indices, residual indices) that row blocks [r0, r1) own, each sorted."""
    ptr = bs.row_cell_ptr.astype(np.int64)
    _, start, end, _, _ = cells(bs)
    c0, c1 = int(ptr[r0]), int(ptr[r1])
    v = [np.arange(start[c], end[c]) for c in range(c0, c1)]
    v = np.sort(np.concatenate(v)) if v else np.zeros(0, np.int64)
    b0 = int(bs.row_block_pos[r0])
    b1 = int(bs.row_block_pos[r1 - 1]) + int(bs.row_block_size[r1 - 1])
    return v.astype(np.int64), np.arange(b0, b1, dtype=np.int64)


def class_bytes(bs, r0, r1, k, streams):
    """The value indices of class k (of `streams` classes) that row blocks [r0, r1) own, sorted."""
    row, start, end, cls, _ = cells(bs)
    m = (row >= r0) & (row < r1)
    if streams == 2:
        m &= cls == k
    v = [np.arange(a, b) for a, b in zip(start[m], end[m])]
    return np.sort(np.concatenate(v)).astype(np.int64) if v else np.zeros(0, np.int64)


def cell_mask(bs, extent):
    """True where a double of the value array belongs to a cell."""
    _, start, end, _, _ = cells(bs)
    d = np.zeros(extent + 1, dtype=np.int64)
    np.add.at(d, start, 1)
    np.add.at(d, end, -1)
    return np.cumsum(d)[:extent] > 0


def column_of_value(bs, extent):
    """The scalar column of every double of the value array that belongs to a cell (-1 elsewhere)."""
    row, start, end, _, col = cells(bs)
    out = np.full(extent, -1, dtype=np.int64)
    csz = bs.col_block_size.astype(np.int64)
    cpos = bs.col_block_pos.astype(np.int64)
    for w in np.unique(csz[col]):
        idx = np.flatnonzero(csz[col] == w)
        for h in np.unique(bs.row_block_size[row[idx]]):
            sub = idx[bs.row_block_size[row[idx]] == h]
            offs = np.arange(int(h) * int(w))
            out[(start[sub][:, None] + offs[None, :]).reshape(-1)] = (cpos[col[sub]][:, None] + (offs % int(w))[None, :]).reshape(-1)
    return out


def device_image(bs, host_values, host_b, scale=None, before_values=None, before_b=None):
    """What HBM must hold after _end: (values, residuals, mask).  Every double of a cell equals the host's, times scale[column] where a
    scale is given — one fp64 multiply, so bit-equal to numpy's product; every residual equals the host's.  Doubles of the value array that
    belong to no cell are unconstrained: mask is False there, and the image carries before_values (what the device held) for reading."""
    extent = bs.values_extent()
    mask = cell_mask(bs, extent)
    values = np.array(before_values[:extent], dtype=np.float64) if before_values is not None else np.full(extent, np.nan)
    v = np.asarray(host_values, dtype=np.float64)[:extent]
    if scale is not None:
        colv = column_of_value(bs, extent)
        v = np.where(mask, v * np.asarray(scale, dtype=np.float64)[np.maximum(colv, 0)], v)
    values[mask] = v[mask]
    return values, np.array(host_b, dtype=np.float64), mask


def same_bits(a, b):
    """Bit equality of two float64 arrays (NaN payloads and signed zeros included)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
