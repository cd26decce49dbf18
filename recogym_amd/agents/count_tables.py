"""What OrganicCount and BanditCount share: P x P tables of integer counters and the reduction of a whole log to them.

The reference keeps dense float64 arrays and adds a dense outer product per train call (organic_count.py:74-82,
bandit_count.py:49-62).  All its numbers are integers, so here a table is

* on the host a sparse int64 matrix (coordinate updates, summed lazily): P = 10^4 stays cheap, and
* on the device a dense int64 tensor that `rg_count_train` adds a sorted log to (include/recogym_hip.h) — the log never
  crosses PCIe.

The two parts add up to the reference's array; `dense()` materialises it as float64 on demand.

The train calls a log stands for (bench_agents.py:90-190, `_train_from_dataframe`): one per bandit row with the organic rows
since the user's previous bandit row as its session, and one without an action for the organic rows that end a user.  A session
id therefore starts at every new user and after every bandit row.
"""
import ctypes as C

import numpy as np
from scipy import sparse

from .. import _abi

# tables of at most this many bytes are materialised densely / allocated on the device (8 P^2 bytes each: 0.8 GB at P = 10^4)
MAX_TABLE_BYTES = 4 << 30


def check_table_size(P, what):
    need = 8 * int(P) * int(P)
    if need > MAX_TABLE_BYTES:
        raise MemoryError(f'{what}: a {P} x {P} table of 64-bit counters needs {need / 2**30:.1f} GiB '
                          f'(limit {MAX_TABLE_BYTES / 2**30:.0f} GiB), as the dense arrays of the reference would')


class CountTable:
    """One P x P table of counters = host part (sparse) + device part (dense int64 tensor, or None)."""

    def __init__(self, P):
        self.P = int(P)
        self.host = sparse.csr_matrix((self.P, self.P), dtype=np.int64)
        self.dev = None
        self._rows, self._cols, self._vals = [], [], []
        self._pending = 0

    # -- host part ---------------------------------------------------------------------------------------
    def add(self, rows, cols, vals):
        rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
        if rows.size == 0:
            return
        self._rows.append(rows)
        self._cols.append(np.atleast_1d(np.asarray(cols, dtype=np.int64)))
        self._vals.append(np.broadcast_to(np.asarray(vals, dtype=np.int64), rows.shape))
        self._pending += rows.size
        if len(self._rows) >= 4096:
            self._settle()

    def add_row(self, row, val):
        """table[row, :] += val — what NumPy's `table[None, row] += val` does (bandit_count.py:57 with ix = None)."""
        self.add(np.full(self.P, int(row)), np.arange(self.P), int(val))

    def _settle(self):
        if self._rows:
            upd = sparse.coo_matrix((np.concatenate(self._vals), (np.concatenate(self._rows), np.concatenate(self._cols))),
                                    shape=(self.P, self.P), dtype=np.int64).tocsr()      # duplicates are summed
            self.host = (self.host + upd).tocsr()
            self._rows, self._cols, self._vals = [], [], []
            self._pending = 0
        return self.host

    def set_dense(self, array):
        """Replace the whole table (BanditCount.load)."""
        a = np.asarray(array)
        assert a.shape == (self.P, self.P)
        self._rows, self._cols, self._vals = [], [], []
        self.host = sparse.csr_matrix(np.rint(a).astype(np.int64))
        self.dev = None

    # -- device part -------------------------------------------------------------------------------------
    def device(self, device):
        """The device tensor (allocated at first use); the host part is added to it and emptied."""
        import torch
        if self.dev is None:
            check_table_size(self.P, 'device count table')
            self.dev = torch.zeros((self.P, self.P), dtype=torch.int64, device=device)
        h = self._settle().tocoo()
        if h.nnz:
            self.dev.index_put_((torch.from_numpy(h.row.astype(np.int64)).to(self.dev.device),
                                 torch.from_numpy(h.col.astype(np.int64)).to(self.dev.device)),
                                torch.from_numpy(h.data).to(self.dev.device), accumulate=True)
            self.host = sparse.csr_matrix((self.P, self.P), dtype=np.int64)
        return self.dev

    # -- reading -----------------------------------------------------------------------------------------
    def dense(self):
        check_table_size(self.P, 'dense count table')
        out = self._settle().toarray().astype(np.float64)
        if self.dev is not None:
            out += self.dev.cpu().numpy()
        return out

    def coo(self):
        """-> (rows, cols, values) of the non-zero cells, row-major order."""
        if self.dev is not None:
            m = sparse.csr_matrix(self.dev.cpu().numpy()) + self._settle()
        else:
            m = self._settle()
        m = m.tocsr()
        m.sum_duplicates()
        m.eliminate_zeros()
        m.sort_indices()
        c = m.tocoo()
        return c.row.astype(np.int64), c.col.astype(np.int64), c.data.astype(np.int64)

    def rows_dense(self, lo, hi):
        """Rows lo .. hi-1 as a float64 array (host part only: callers fold the device part in first or have none)."""
        assert self.dev is None
        return self._settle()[lo:hi].toarray().astype(np.float64)


# ----------------------------------------------------------------------------------------------------------
# a log as arrays
# ----------------------------------------------------------------------------------------------------------
def log_arrays(log):
    """DataFrame of generate_logs / dict of Simulator.log_columns() -> (u, is_bandit, v, a, click) int64 / bool arrays."""
    from .feature_feed import _columns_of
    u, is_b, v, a, c, _ = _columns_of(log)
    return u, is_b, v, a, np.nan_to_num(np.asarray(c, dtype=np.float64)) != 0


def organic_updates(u, is_b, v, P, sessions=None):
    """The cells b b^T of every session touches -> (rows, cols, values): b[p] = views of p in the session; every maximal run of
    organic rows inside a user is a session (it ends in a bandit row, or ends the user: the call without an action).
    `sessions(sid)` (optional) -> the ids of the sessions that count, given every row's session id (a bandit row carries the
    id of the session it closes)."""
    n = len(u)
    empty = np.zeros(0, dtype=np.int64)
    if n == 0 or is_b.all():
        return empty, empty, empty
    start = np.r_[True, u[1:] != u[:-1]] | np.r_[False, is_b[:-1]]
    sid = np.cumsum(start) - 1
    org = ~is_b
    if sessions is not None:
        org = org & np.isin(sid, sessions(sid))
        if not org.any():
            return empty, empty, empty
    if v[org].min() < 0 or v[org].max() >= P:
        raise ValueError(f'the log views products outside [0, {P})')
    key, cnt = np.unique(sid[org] * P + v[org], return_counts=True)          # (session, product) -> views, sessions ascending
    s, p = key // P, key % P
    first = np.r_[True, s[1:] != s[:-1]]
    seg = np.flatnonzero(first)                                              # first entry of every session
    m = np.diff(np.r_[seg, len(s)])                                          # distinct products per session
    m_of = np.repeat(m, m)
    seg_of = np.repeat(seg, m)
    total = int(m_of.sum())
    rep = np.repeat(np.arange(len(s)), m_of)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(m_of) - m_of, m_of)
    other = seg_of[rep] + within
    return p[rep], p[other], cnt[rep].astype(np.int64) * cnt[other]


def bandit_updates(u, is_b, v, a, click, P, carry):
    """BanditCount's train calls -> (ix, action, click) per bandit row, the new carry.  ix = the agent's last_product_viewed
    BEFORE the row's own session is looked at (bandit_count.py:54-56): the last organic view in front of the PREVIOUS bandit
    row of the log, whichever user that row belongs to (a user's trailing organic rows are a call without an action and do not
    move it); `carry` (None = never set) where the log has none.  ix = -1 stands for None."""
    n = len(u)
    b_rows = np.flatnonzero(is_b)
    if b_rows.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), carry
    if a[b_rows].min() < 0 or a[b_rows].max() >= P:
        raise ValueError(f'the log has actions outside [0, {P})')
    new_user = np.r_[True, u[1:] != u[:-1]]
    # organic rows directly followed by a bandit row of the same user: the views last_product_viewed moves to
    moves = np.flatnonzero(np.r_[~is_b[:-1] & is_b[1:] & ~new_user[1:], False]) if n > 1 else np.zeros(0, dtype=np.int64)
    if moves.size and (v[moves].min() < 0 or v[moves].max() >= P):
        raise ValueError(f'the log views products outside [0, {P})')
    prev_b = np.r_[-1, b_rows[:-1]]                                          # the previous bandit row of the log
    k = np.searchsorted(moves, prev_b, side='left') - 1                      # the last move in front of it
    c0 = -1 if carry is None else int(carry)
    ix = np.where(k >= 0, v[moves[np.maximum(k, 0)]] if moves.size else c0, c0).astype(np.int64)
    # the last bandit row's own call moves it once more
    last = np.searchsorted(moves, b_rows[-1], side='left') - 1
    new_carry = carry if last < 0 else int(v[moves[last]])
    return ix, a[b_rows].astype(np.int64), click[b_rows], new_carry


# ----------------------------------------------------------------------------------------------------------
# the online protocol under a row filter (evaluate_agent's evolution steps)
# ----------------------------------------------------------------------------------------------------------
def online_arrays(log):
    """-> (u, is_b, v, a, click, phantom): log_arrays plus the phantom flag of every row — the `phantom` entry of a column
    dict where it has one, else no row is a phantom row (a log of evaluate_agent's own loop has none)."""
    u, is_b, v, a, click = log_arrays(log)
    ph = log.get('phantom') if isinstance(log, dict) else None
    return u, is_b, v, a, click, (np.zeros(len(u), dtype=bool) if ph is None else np.asarray(ph).astype(bool))


def counted_rows(is_b, phantom=None, mask=None):
    """The rows that stand for a train call: bandit rows that are not phantom rows and that the mask lets through."""
    out = np.asarray(is_b, dtype=bool).copy()
    if phantom is not None:
        out &= ~np.asarray(phantom, dtype=bool)
    if mask is not None:
        out &= np.asarray(mask) != 0
    return out


def online_organic_updates(u, is_b, v, P, counted):
    """OrganicCount's train calls at the counted rows -> (rows, cols, values): b b^T of every session a counted row closes (a
    session in front of any other bandit row, or at the end of a user, is never counted)."""
    return organic_updates(u, is_b, v, P, sessions=lambda sid: sid[counted])


def online_bandit_updates(u, is_b, v, a, click, P, counted, carry):
    """BanditCount's train calls at the counted rows -> (ix, action, click) per counted row and the new carry: last_product_viewed
    walks over the counted rows in log order, across users — ix is its value before the row, then it moves to the view directly
    in front of the row where that row is an organic row of the same user (the last view of the row's own session).  ix = -1
    stands for None; any number of rows can meet it."""
    rows = np.flatnonzero(counted)
    if rows.size == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool), carry
    if a[rows].min() < 0 or a[rows].max() >= P:
        raise ValueError(f'the log has actions outside [0, {P})')
    prev = np.maximum(rows - 1, 0)
    has = (rows > 0) & ~is_b[prev] & (u[prev] == u[rows])
    sv = np.where(has, v[prev], -1).astype(np.int64)
    if sv.max() >= P:
        raise ValueError(f'the log views products outside [0, {P})')
    pos = np.maximum.accumulate(np.where(sv >= 0, np.arange(rows.size), -1))
    before = np.r_[-1, pos[:-1]]
    c0 = -1 if carry is None else int(carry)
    ix = np.where(before >= 0, sv[np.maximum(before, 0)], c0).astype(np.int64)
    new_carry = carry if pos[-1] < 0 else int(sv[pos[-1]])
    return ix, a[rows].astype(np.int64), click[rows], new_carry


# ----------------------------------------------------------------------------------------------------------
# the device reduction
# ----------------------------------------------------------------------------------------------------------
def device_present():
    try:
        import torch
    except ImportError:
        return False
    return torch.cuda.is_available() and _abi.load().rg_device_count() > 0


def as_device_log(log):
    """A Simulator or a DeviceLog -> DeviceLog; anything else -> None."""
    from ..sim import DeviceLog, Simulator
    if isinstance(log, Simulator):
        return log.device_log()
    return log if isinstance(log, DeviceLog) else None


def columns_to_device_log(u, is_b, v, a, click, P, device, t=None, phantom=None):
    """Log columns -> a DeviceLog (rows in the given order; every run of equal u is a user).  `t`: the rows' event indices (0
    where not given: enough for everything that draws nothing); `phantom`: the rows that carry the phantom flag."""
    import torch
    from ..sim import DeviceLog
    n = len(u)
    raw = np.zeros((n, 4), dtype=np.uint32)
    raw[:, 0] = u.astype(np.uint32)
    if t is not None:
        raw[:, 1] = np.asarray(t).astype(np.uint32)
    raw[:, 2] = (np.where(is_b, a, v).astype(np.uint32) | np.where(is_b, _abi.RG_EV_BANDIT, 0).astype(np.uint32)
                 | np.where(is_b & click, _abi.RG_EV_CLICK, 0).astype(np.uint32))
    if phantom is not None:
        raw[:, 2] |= np.where(np.asarray(phantom, dtype=bool), _abi.RG_EV_PHANTOM, 0).astype(np.uint32)
    start = np.flatnonzero(np.r_[True, u[1:] != u[:-1]]) if n else np.zeros(0, dtype=np.int64)
    offsets = np.r_[start, n].astype(np.int64)
    return DeviceLog(torch.from_numpy(raw.view(np.int32)).to(device), torch.from_numpy(offsets).to(device), None, 0, int(P), None)


def count_train(dl, P, co=None, pulls=None, clicks=None, carry=None):
    """rg_count_train on a DeviceLog: adds the log to the given int64 device tables -> (new carry, stats dict)."""
    import torch
    lib = _abi.load()
    if int(dl.num_products) != int(P):
        raise ValueError(f'the log has {dl.num_products} products, the agent {P}')
    device = dl.rows.device
    n_users = int(dl.offsets.numel()) - 1
    tabs = _abi.RgCountTables(num_products=int(P), reserved=0,
                              co_counts=None if co is None else co.data_ptr(),
                              pulls=None if pulls is None else pulls.data_ptr(),
                              clicks=None if clicks is None else clicks.data_ptr())
    with torch.cuda.device(device):
        need = lib.rg_count_workspace_bytes()
        ws = torch.zeros(need, dtype=torch.uint8, device=device)
        cr = torch.tensor([-1 if carry is None else int(carry), -1, 0, 0], dtype=torch.int64, device=device)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _abi.check(lib.rg_count_train(C.byref(tabs), dl.rows.data_ptr(), dl.offsets.data_ptr(), n_users, cr.data_ptr(),
                                      ws.data_ptr(), need, stream), 'rg_count_train')
        out = cr.cpu().numpy()
        st = ws.view(torch.int64)[:4].cpu().numpy()
    return (None if out[0] < 0 else int(out[0])), dict(updates=int(st[1]), global_atomics=int(st[2]), none_row=int(out[1]))


def count_train_online(dl, P, co=None, pulls=None, clicks=None, carry=None, mask=None):
    """rg_count_train_online on a DeviceLog: the train calls at the counted rows (bandit, not phantom, let through by `mask`: a
    uint8 / bool device tensor with one entry per row of the log, or None) added to the given int64 device tables -> (new
    carry, stats dict)."""
    import torch
    lib = _abi.load()
    if int(dl.num_products) != int(P):
        raise ValueError(f'the log has {dl.num_products} products, the agent {P}')
    device = dl.rows.device
    n_users = int(dl.offsets.numel()) - 1
    if mask is not None:
        if int(mask.numel()) != int(dl.rows.shape[0]):
            raise ValueError(f'the mask has {int(mask.numel())} entries, the log {int(dl.rows.shape[0])} rows')
        mask = mask.to(device=device, dtype=torch.uint8).contiguous()
    tabs = _abi.RgCountTables(num_products=int(P), reserved=0,
                              co_counts=None if co is None else co.data_ptr(),
                              pulls=None if pulls is None else pulls.data_ptr(),
                              clicks=None if clicks is None else clicks.data_ptr())
    with torch.cuda.device(device):
        need = lib.rg_count_online_workspace_bytes(int(P), n_users)
        ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
        cr = torch.tensor([-1 if carry is None else int(carry)], dtype=torch.int64, device=device)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _abi.check(lib.rg_count_train_online(C.byref(tabs), dl.rows.data_ptr(), dl.offsets.data_ptr(), n_users,
                                             None if mask is None else mask.data_ptr(), cr.data_ptr(), ws.data_ptr(), need, stream),
                   'rg_count_train_online')
        out = int(cr.item())
        st = ws[:4].cpu().numpy()
    return (None if out < 0 else out), dict(updates=int(st[1]), global_atomics=int(st[2]))


def count_policy(P, kind, co=None, pulls=None, clicks=None):
    """rg_count_policy -> (action int32 [P], winning clicks, winning pulls) as host arrays."""
    import torch
    lib = _abi.load()
    t0 = co if co is not None else pulls
    device = t0.device
    tabs = _abi.RgCountTables(num_products=int(P), reserved=0,
                              co_counts=None if co is None else co.data_ptr(),
                              pulls=None if pulls is None else pulls.data_ptr(),
                              clicks=None if clicks is None else clicks.data_ptr())
    with torch.cuda.device(device):
        action = torch.empty(P, dtype=torch.int32, device=device)
        wc = torch.zeros(P, dtype=torch.int64, device=device)
        wn = torch.zeros(P, dtype=torch.int64, device=device)
        stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        _abi.check(lib.rg_count_policy(C.byref(tabs), int(kind), action.data_ptr(), wc.data_ptr(), wn.data_ptr(), stream),
                   'rg_count_policy')
        return action.cpu().numpy(), wc.cpu().numpy(), wn.cpu().numpy()


def host_argmax_rows(P, value_rows):
    """First index of the maximum of every row, rows produced a block at a time by value_rows(lo, hi) (float64 (hi - lo, P))."""
    table = np.empty(P, dtype=np.int64)
    win = np.empty(P, dtype=np.float64)
    step = max(1, min(P, (32 << 20) // (8 * P)))
    for lo in range(0, P, step):
        hi = min(P, lo + step)
        x = value_rows(lo, hi)
        table[lo:hi] = x.argmax(axis=1)
        win[lo:hi] = x[np.arange(hi - lo), table[lo:hi]]
    return table, win
