"""Upstream-gradient masks of tests/test_gpu_deform_live_rows.py and the numbers the deformation backward must report for them: plain
torch on the CPU, no device and no library.

A mask is an [n] 0/1 vector that multiplies the upstream weights of every output (`upstream_mask` of test_gpu_deform._grads_pair); the
`one_output` mask is five such vectors, one per output, and a row is live when ANY of them is set (the packing stage ORs over all packed
columns).  The row-list form of the backward pads its list to whole units of ROW_UNIT entries; the tile form walks 32-row tiles."""
import torch

TILE = 32
ROW_UNIT = 128            # row_pad of csrc/deform.hip::bwd_lists at C = 16 and 32 (max(128, 2048 / C))
SIZES = (31, 300, 4100)   # one partial tile; ten tiles, the last partial; 129 tiles, the last with four rows
MASKS = ("none", "first", "last", "mid", "tail_tile", "pad-1", "pad", "pad+1", "stride32", "stride33", "even", "all", "one_output")
MASKS_AT_31 = ("none", "first", "last", "even", "all")
OUTPUTS = ("xyz", "scales", "rot", "opacity", "shs")
ONE_OUTPUT_GROUPS = ("xyz", "rot", "opacity", "shs")      # group g of the live rows has non-zero weights in this output only

# live rows of every (mask, n) the tests use: a change to a mask builder cannot empty a case unnoticed
LIVE_ROWS = {
    31: {"none": 0, "first": 1, "last": 1, "even": 16, "all": 31},
    300: {"none": 0, "first": 1, "last": 1, "mid": 1, "tail_tile": 12, "pad-1": 127, "pad": 128, "pad+1": 129, "stride32": 10,
          "stride33": 10, "even": 150, "all": 300, "one_output": 75},
    4100: {"none": 0, "first": 1, "last": 1, "mid": 1, "tail_tile": 4, "pad-1": 127, "pad": 128, "pad+1": 129, "stride32": 129,
           "stride33": 125, "even": 2050, "all": 4100, "one_output": 1025},
}


def masks_for(n):
    return MASKS_AT_31 if n == 31 else MASKS


def cases(sizes=SIZES):
    return [(n, name) for n in sizes for name in masks_for(n)]


def _rows(idx, n):
    m = torch.zeros(n)
    m[idx] = 1.0
    return m


def row_mask(name, n):
    """The [n] 0/1 vector of live rows of mask `name` (for `one_output`: the OR of its five vectors)."""
    assert n % TILE != 0, "the last tile is meant to be partial"
    r = torch.arange(n)
    if name == "none":
        return torch.zeros(n)
    if name == "first":
        return _rows([0], n)
    if name == "last":
        return _rows([n - 1], n)
    if name == "mid":
        return _rows([45], n)
    if name == "tail_tile":
        return (r >= n // TILE * TILE).float()
    if name in ("pad-1", "pad", "pad+1"):
        k = ROW_UNIT + {"pad-1": -1, "pad": 0, "pad+1": 1}[name]
        return _rows(torch.randperm(n, generator=torch.Generator().manual_seed(1000 + k))[:k], n)
    if name == "stride32":
        return (r % 32 == 0).float()
    if name == "stride33":
        return (r % 33 == 0).float()
    if name == "even":
        return (r % 2 == 0).float()
    if name == "all":
        return torch.ones(n)
    if name == "one_output":
        return (r % 4 == 1).float()
    raise KeyError(name)


def output_masks(name, n):
    """Five [n] 0/1 vectors, one per output of deform() (OUTPUTS): the same vector for every mask but `one_output`, where the live rows
    (r % 4 == 1) fall into four groups ((r // 4) % 4) with non-zero weights in xyz only, rotation only, opacity only and SH only;
    the scales get no upstream at all."""
    m = row_mask(name, n)
    if name != "one_output":
        return [m] * 5
    group = (torch.arange(n) // 4) % 4
    per = {o: m * (group == g).float() for g, o in enumerate(ONE_OUTPUT_GROUPS)}
    return [per.get(o, torch.zeros(n)) for o in OUTPUTS]


def expected(name, n):
    """(live rows, distinct live 32-row tiles, padded length of the row list) of mask `name` at `n` rows."""
    live = torch.zeros(n, dtype=torch.bool)
    for m in output_masks(name, n):
        live |= m != 0
    rows = torch.nonzero(live).squeeze(1)
    n_live = int(rows.numel())
    return n_live, int(torch.unique(rows // TILE).numel()), -(-n_live // ROW_UNIT) * ROW_UNIT


def tiles_total(n):
    """32-row tiles of the padded set (N rounded up to 128 rows): what the backward walks with skip_dead = 0."""
    return -(-n // 128) * 4
