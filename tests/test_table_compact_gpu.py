"""The voxel table's compaction kernel (geo4d_amd/csrc/voxel_table.h table_compact_kernel) in both its forms, on fabricated tables: keys
only through ops.tsdf_compact, (key, slot) pairs through geo4d_fuse_compact. The scene tests only ever reach it with room for every
key and with capacities that are whole 4 096-slot tiles; here the capacities are 1, one round of one workgroup, exactly one tile and
two workgroups (so the base comes from the atomic on the count), and the limit is also put at half the count: into output buffers of
exactly that many rows, and into larger pre-filled ones, where a row written past the limit would show."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CAPACITIES = (1, 256, 4096, 8192)
PATTERNS = ("empty", "full", "last", "half")
SENTINEL = -7                                                   # no key (keys are >= 0) and no slot


def _table(capacity, pattern, dev):
    """(table int64 [capacity] with -1 for empty, the occupied slots): distinct keys below 2^63."""
    g = torch.Generator().manual_seed(capacity)
    occupied = {"empty": torch.zeros(capacity, dtype=torch.bool), "full": torch.ones(capacity, dtype=torch.bool),
                "last": torch.arange(capacity) == capacity - 1, "half": torch.rand(capacity, generator=g) < 0.5}[pattern]
    keys = torch.arange(capacity, dtype=torch.int64) * 1_000_003 + (1 << 40) + 12345
    table = torch.where(occupied, keys[torch.randperm(capacity, generator=g)], torch.full((capacity,), -1, dtype=torch.int64))
    return table.to(dev), occupied.nonzero().reshape(-1).to(dev)


def _fuse_workspace(lib, table):
    """The table followed by the (mean) accumulator words: geo4d_fuse_workspace bytes."""
    need = lib.geo4d_fuse_workspace(table.numel(), 0)
    ws = torch.zeros(need // 8, device=table.device, dtype=torch.int64)
    ws[:table.numel()] = table
    return ws, need


def _pairs(lib, ws, need, capacity, keys, slots, max_pairs):
    from geo4d_amd import _lib, ops
    count = torch.full((1,), SENTINEL, device=ws.device, dtype=torch.int64)
    _lib.check(lib.geo4d_fuse_compact(capacity, 0, keys.data_ptr(), slots.data_ptr(), max_pairs, count.data_ptr(), ws.data_ptr(), need,
                                      ops._stream()), "geo4d_fuse_compact")
    return int(count)


def _check_rows(table, keys, slots=None):
    """Every row is a distinct occupied key of the table, and with slots the slot that holds it."""
    assert (keys >= 0).all() and keys.unique().numel() == keys.numel()
    assert torch.isin(keys, table[table >= 0]).all()
    if slots is not None:
        assert ((slots >= 0) & (slots < table.numel())).all()
        assert torch.equal(table[slots], keys)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("capacity", CAPACITIES)
def test_room_for_all(capacity, pattern):
    from geo4d_amd import _lib, ops
    lib, dev = _lib.load(), torch.device("cuda:0")
    table, occupied = _table(capacity, pattern, dev)
    n, want = occupied.numel(), torch.sort(table[occupied]).values
    keys, count = ops.tsdf_compact(table)
    assert int(count) == n and keys.numel() == capacity
    assert torch.equal(torch.sort(keys[:n]).values, want)
    ws, need = _fuse_workspace(lib, table)
    keys = torch.full((capacity,), SENTINEL, device=dev, dtype=torch.int64)
    slots = torch.full((capacity,), SENTINEL, device=dev, dtype=torch.int64)
    assert _pairs(lib, ws, need, capacity, keys, slots, capacity) == n
    assert torch.equal(torch.sort(keys[:n]).values, want)
    assert torch.equal(table[slots[:n]], keys[:n])
    assert (keys[n:] == SENTINEL).all() and (slots[n:] == SENTINEL).all()
    assert torch.equal(ws[:capacity], table) and not ws[capacity:].any()          # the table is only read


@pytest.mark.parametrize("pattern", ("full", "half"))
@pytest.mark.parametrize("capacity", CAPACITIES)
def test_limit_at_half_the_count(capacity, pattern):
    """max_keys / max_pairs below the count: the count still says how many there were, and only `limit` rows are written. A capacity
    of 1 has no half: its limit is 1 (ops.tsdf_compact asks for one row at least)."""
    from geo4d_amd import _lib, ops
    lib, dev = _lib.load(), torch.device("cuda:0")
    table, occupied = _table(capacity, pattern, dev)
    n = occupied.numel()
    limit = max(n // 2, 1)
    written = min(limit, n)
    # keys only, in a buffer of exactly `limit` rows
    keys, count = ops.tsdf_compact(table, max_keys=limit)
    assert int(count) == n and keys.numel() == limit
    _check_rows(table, keys[:written])
    # pairs, in two buffers of exactly `limit` rows
    ws, need = _fuse_workspace(lib, table)
    keys = torch.full((limit,), SENTINEL, device=dev, dtype=torch.int64)
    slots = torch.full((limit,), SENTINEL, device=dev, dtype=torch.int64)
    assert _pairs(lib, ws, need, capacity, keys, slots, limit) == n
    _check_rows(table, keys[:written], slots[:written])
    assert (keys[written:] == SENTINEL).all() and (slots[written:] == SENTINEL).all()
    # both forms into pre-filled buffers with room for all: rows past the limit keep their sentinel
    keys = torch.full((capacity,), SENTINEL, device=dev, dtype=torch.int64)
    slots = torch.full((capacity,), SENTINEL, device=dev, dtype=torch.int64)
    assert _pairs(lib, ws, need, capacity, keys, slots, limit) == n
    _check_rows(table, keys[:written], slots[:written])
    assert (keys[written:] == SENTINEL).all() and (slots[written:] == SENTINEL).all()
    keys.fill_(SENTINEL)
    count = torch.full((1,), SENTINEL, device=dev, dtype=torch.int64)
    _lib.check(lib.geo4d_tsdf_compact(capacity, keys.data_ptr(), limit, count.data_ptr(), table.data_ptr(), capacity * 8, ops._stream()),
               "geo4d_tsdf_compact")
    assert int(count) == n
    _check_rows(table, keys[:written])
    assert (keys[written:] == SENTINEL).all()
    assert torch.equal(ws[:capacity], table)
