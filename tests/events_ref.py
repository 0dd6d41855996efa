"""Spectrum events (include/fsea.h: fsea_events_*) restated in numpy, twice: runs_of() / link() vectorised (a segment per
run over the hit cells; the touching pairs by binary search, the components by scipy's connected_components), and
runs_of_loops() / link_loops(), the definitions read out literally (a loop over the cells of a row; every pair of runs tested
for touch, a union by relabelling) for small shapes.  tests/test_events_host.py holds the two against each other and
fsea_events_link against both; the GPU tier compares the kernels with runs_of() and paint() bit for bit.  The levels are
tests/cfar_ref.py's; sums are int64 and wrap as numpy's do."""
import numpy as np

from tests import cfar_ref

MAX_WIDTH, MAX_GAP_COLS, MAX_GAP_ROWS, NO_EVENT = 1 << 20, 64, 1 << 16, 0xFFFFFFFF
RUN = np.dtype([("row", "<u4"), ("first", "<u4"), ("last", "<u4"), ("hits", "<u4"), ("peak", "<i4"), ("peak_col", "<u4"),
                ("level_sum", "<i8")])
EVENT = np.dtype([("row_first", "<u4"), ("row_last", "<u4"), ("col_first", "<u4"), ("col_last", "<u4"), ("runs", "<u4"),
                  ("peak", "<i4"), ("peak_row", "<u4"), ("peak_col", "<u4"), ("hits", "<u8"), ("level_sum", "<i8")])


def runs_of(mask, levels=None, gap_cols=0, row0=0):
    """The runs of a 2-D mask (a hit is a byte that is not 0), sorted by (row, first): a structured array of dtype RUN."""
    mask = np.asarray(mask)
    rows, cols = np.nonzero(mask)                              # row-major: sorted by (row, column)
    out = np.zeros(0, RUN)
    if rows.size == 0:
        return out
    start = np.ones(rows.size, bool)
    start[1:] = (rows[1:] != rows[:-1]) | (cols[1:] - cols[:-1] - 1 > gap_cols)
    at = np.flatnonzero(start)
    end = np.append(at[1:], rows.size) - 1
    out = np.zeros(at.size, RUN)
    out["row"], out["first"], out["last"], out["hits"] = rows[at] + row0, cols[at], cols[end], end - at + 1
    out["peak_col"] = cols[at]
    if levels is not None:
        lv = cfar_ref.levels_of(levels)[rows, cols]
        peak = np.maximum.reduceat(lv, at)
        seg = np.cumsum(start) - 1
        out["peak"], out["level_sum"] = peak, np.add.reduceat(lv, at)
        out["peak_col"] = np.minimum.reduceat(np.where(lv == peak[seg], cols, MAX_WIDTH), at)
    return out


def runs_of_loops(mask, levels=None, gap_cols=0, row0=0):
    """The definition literally: going up the columns, a run starts at a hit and continues through every further hit that has
    at most gap_cols non-hit columns before it."""
    mask = np.asarray(mask)
    lv = None if levels is None else cfar_ref.levels_of(levels)
    found = []
    for r in range(mask.shape[0]):
        run, last_hit = None, None
        for c in range(mask.shape[1]):
            if mask[r, c] == 0:
                continue
            if last_hit is None or c - last_hit - 1 > gap_cols:
                run = dict(row=r + row0, first=c, last=c, hits=0, peak=None, peak_col=c, level_sum=0)
                found.append(run)
            level = 0 if lv is None else int(lv[r, c])
            run["last"], run["hits"], run["level_sum"] = c, run["hits"] + 1, run["level_sum"] + level
            if run["peak"] is None or level > run["peak"]:
                run["peak"], run["peak_col"] = level, c
            last_hit = c
    out = np.zeros(len(found), RUN)
    for i, run in enumerate(found):
        out[i] = (run["row"], run["first"], run["last"], run["hits"], run["peak"] if lv is not None else 0,
                  run["peak_col"] if lv is not None else run["first"], run["level_sum"])
    return out


def touch(a, b, gap_cols, gap_rows):
    """Run a in row ra and run b in row rb > ra."""
    return (int(b["row"]) > int(a["row"]) and int(b["row"]) - int(a["row"]) <= gap_rows + 1
            and int(a["first"]) <= int(b["last"]) + gap_cols and int(b["first"]) <= int(a["last"]) + gap_cols)


def _events_of(runs, label, min_rows, min_cols, min_hits):
    """label[i]: any number that is the same for the runs of one event.  (events that pass the filters, event_of_run)."""
    n = runs.size
    if n == 0:
        return np.zeros(0, EVENT), np.zeros(0, np.uint32)
    _, first_run, inverse = np.unique(label, return_index=True, return_inverse=True)
    rank = np.empty(first_run.size, np.int64)
    rank[np.argsort(first_run, kind="stable")] = np.arange(first_run.size)     # events in the order of their first runs
    ev = rank[inverse.ravel()]
    order = np.argsort(ev, kind="stable")                                      # within an event: still by (row, first)
    r, at = runs[order], np.flatnonzero(np.diff(ev[order], prepend=-1))
    seg = ev[order]
    events = np.zeros(at.size, EVENT)
    events["row_first"], events["row_last"] = np.minimum.reduceat(r["row"], at), np.maximum.reduceat(r["row"], at)
    events["col_first"], events["col_last"] = np.minimum.reduceat(r["first"], at), np.maximum.reduceat(r["last"], at)
    events["runs"] = np.add.reduceat(np.ones(n, np.int64), at)
    events["hits"] = np.add.reduceat(r["hits"].astype(np.uint64), at)
    events["level_sum"] = np.add.reduceat(r["level_sum"], at)                 # int64: wraps modulo 2^64
    peak = np.maximum.reduceat(r["peak"], at)
    where = r["row"].astype(np.int64) * (2 * MAX_WIDTH) + r["peak_col"]        # lowest row, then lowest column
    best = np.minimum.reduceat(np.where(r["peak"] == peak[seg], where, np.iinfo(np.int64).max), at)
    events["peak"], events["peak_row"], events["peak_col"] = peak, best // (2 * MAX_WIDTH), best % (2 * MAX_WIDTH)
    keep = ((events["row_last"].astype(np.int64) - events["row_first"] + 1 >= min_rows)
            & (events["col_last"].astype(np.int64) - events["col_first"] + 1 >= min_cols) & (events["hits"] >= min_hits))
    number = np.where(keep, np.cumsum(keep) - 1, NO_EVENT).astype(np.uint32)
    return events[keep], number[ev]


def link(runs, gap_cols=0, gap_rows=0, min_rows=1, min_cols=1, min_hits=1):
    """(events, event_of_run) of runs sorted by (row, first) and disjoint within a row."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    runs = np.asarray(runs, RUN)
    n = runs.size
    if n == 0:
        return _events_of(runs, np.zeros(0, np.int64), min_rows, min_cols, min_hits)
    big = 4 * MAX_WIDTH
    row, first, last = runs["row"].astype(np.int64), runs["first"].astype(np.int64), runs["last"].astype(np.int64)
    key_first, key_last = row * big + first + MAX_WIDTH, row * big + last + MAX_WIDTH      # both sorted: the runs of a row are disjoint
    present = np.unique(row)
    pa, pb = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for dr in range(1, gap_rows + 2):
        if dr > present[-1] - present[0]:
            break
        lo = np.searchsorted(key_last, (row + dr) * big + first - gap_cols + MAX_WIDTH, "left")     # last_b + G >= first_a
        hi = np.searchsorted(key_first, (row + dr) * big + last + gap_cols + MAX_WIDTH, "right")    # first_b <= last_a + G
        cnt = np.maximum(hi - lo, 0)
        a = np.repeat(np.arange(n), cnt)
        pa.append(a)
        pb.append(lo[a] + np.arange(a.size) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    pa, pb = np.concatenate(pa), np.concatenate(pb)
    assert (row[pb] > row[pa]).all() and (row[pb] - row[pa] <= gap_rows + 1).all()
    graph = coo_matrix((np.ones(pa.size, np.int8), (pa, pb)), shape=(n, n))
    _, label = connected_components(graph, directed=False)
    return _events_of(runs, label, min_rows, min_cols, min_hits)


def link_loops(runs, gap_cols=0, gap_rows=0, min_rows=1, min_cols=1, min_hits=1):
    """The definition literally: every pair of runs is tested for touch, O(n^2); the events are the connected components."""
    runs = np.asarray(runs, RUN)
    n = runs.size
    label = list(range(n))
    for i in range(n):
        for j in range(n):
            if touch(runs[i], runs[j], gap_cols, gap_rows) and label[i] != label[j]:
                old, new = label[j], label[i]
                label = [new if x == old else x for x in label]
    groups = []                                                                # in the order of their first runs
    for i in range(n):
        if label[i] not in [g[0] for g in groups]:
            groups.append((label[i], [k for k in range(n) if label[k] == label[i]]))
    events, of_run, kept = [], np.full(n, NO_EVENT, np.uint32), 0
    for _, members in groups:
        rs = [runs[k] for k in members]
        peak = max(int(x["peak"]) for x in rs)
        peak_row, peak_col = min((int(x["row"]), int(x["peak_col"])) for x in rs if int(x["peak"]) == peak)
        total = sum(int(x["level_sum"]) for x in rs)
        total = (total + (1 << 63)) % (1 << 64) - (1 << 63)                    # modulo 2^64, as int64
        e = (min(int(x["row"]) for x in rs), max(int(x["row"]) for x in rs), min(int(x["first"]) for x in rs),
             max(int(x["last"]) for x in rs), len(rs), peak, peak_row, peak_col, sum(int(x["hits"]) for x in rs), total)
        if e[1] - e[0] + 1 < min_rows or e[3] - e[2] + 1 < min_cols or e[8] < min_hits:
            continue
        events.append(e)
        of_run[members] = kept
        kept += 1
    return np.array(events, dtype=EVENT), of_run


def paint(runs, values, n_rows, width, row0=0):
    """Columns first .. last of every run with a value that is not 0 and a row in [row0, row0 + n_rows) hold the value."""
    image = np.zeros((n_rows, width), np.uint8)
    for run, value in zip(runs, values):
        r = int(run["row"]) - row0
        if value != 0 and 0 <= r < n_rows:
            image[r, int(run["first"]):int(run["last"]) + 1] = value
    return image
