"""not gpu: the layout arithmetic and the optimizer block table of arena.FlatSpace (the base of ParamArena and FlatTail) against a
per-element definition: element e of the flat buffer belongs to tensor i when offsets[i] <= e < offsets[i] + sizes[i], and a 64-element
block carries the group of the tensor its elements belong to -- or 255 when that tensor is in no group or never gets a gradient."""
import torch

from ecamp_amd import arena

SIZES = [1, 63, 64, 65, 130, 4096]
GROUP = [0, 1, 0, 1, None, 1]      # tensor -> param group (None: in no group)
UNUSED = 2                         # this tensor is `_ecamp_unused`: in a group, but its gradient never arrives


def _owners(offsets, sizes, total):
    """Per element: the tensor it belongs to, -1 for padding; no element may belong to two."""
    own = [-1] * total
    for i, (o, n) in enumerate(zip(offsets, sizes)):
        for e in range(o, o + n):
            assert own[e] == -1, "tensors %d and %d overlap at element %d" % (own[e], i, e)
            own[e] = i
    return own


def _expected_table(own, group_of):
    table = []
    for b in range(len(own) // 64):
        tensors = {t for t in own[64 * b:64 * b + 64] if t >= 0}
        assert len(tensors) == 1, "block %d holds the tensors %s" % (b, sorted(tensors))   # none empty either: every size is >= 1
        g = group_of[tensors.pop()]
        table.append(255 if g is None else g)
    return table


def test_layout_pads_every_tensor_to_64_elements():
    offsets, total = arena.flat_layout(SIZES)
    assert len(offsets) == len(SIZES) and offsets[0] == 0
    assert all(o % 64 == 0 for o in offsets)
    assert total == sum((n + 63) // 64 * 64 for n in SIZES) == 64 + 64 + 64 + 128 + 192 + 4096
    assert total % 64 == 0
    own = _owners(offsets, SIZES, total)
    assert [own.count(i) for i in range(len(SIZES))] == SIZES
    _expected_table(own, [0] * len(SIZES))      # (its assertion: no block holds two tensors)
    assert arena.flat_layout([]) == ([], 0)


def test_block_table_of_integer_spans_matches_the_per_element_definition():
    offsets, total = arena.flat_layout(SIZES)
    live = [g if i != UNUSED else None for i, g in enumerate(GROUP)]
    spans = [(o, n, g) for o, n, g in zip(offsets, SIZES, live) if g is not None]
    table = arena.block_table(total, spans)
    assert table.dtype == torch.uint8 and table.device.type == "cpu" and table.shape == (total // 64,)
    assert table.tolist() == _expected_table(_owners(offsets, SIZES, total), live)
    for o, n, g in zip(offsets, SIZES, live):     # every block of a live grouped tensor carries its group, every other block 255
        assert set(table[o // 64:(o + n + 63) // 64].tolist()) == {255 if g is None else g}
    assert arena.block_table(total, []).tolist() == [255] * (total // 64)


def test_flat_space_block_table_skips_unused_and_ungrouped_parameters():
    params = [torch.nn.Parameter(torch.zeros(n)) for n in SIZES]
    params[UNUSED]._ecamp_unused = True
    space = object.__new__(arena.FlatSpace)        # the layout without the device buffers
    space.params, space.sizes = params, list(SIZES)
    space.offsets, space.total = arena.flat_layout(SIZES)
    space.index = {id(p): i for i, p in enumerate(params)}
    assert [space.span(p) for p in params] == list(zip(space.offsets, SIZES))
    foreign = torch.nn.Parameter(torch.zeros(64))  # a parameter of another space (the classifier's tail beside the arena)
    groups = [{"params": [p for p, g in zip(params, GROUP) if g == 0] + [foreign]}, {"params": [p for p, g in zip(params, GROUP) if g == 1]}]
    table = space.block_table(groups)
    live = [g if i != UNUSED else None for i, g in enumerate(GROUP)]
    assert table.dtype == torch.uint8 and table.device.type == "cpu"
    assert table.tolist() == _expected_table(_owners(space.offsets, SIZES, space.total), live)
    assert sorted(set(table.tolist())) == [0, 1, 255]
