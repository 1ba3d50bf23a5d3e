"""demf_tokens_assemble (csrc/featcache.hip, ``ops.assemble_tokens``) against plain torch indexing on the same device,
bit for bit: every dtype pair, channel widths on each lane layout (4 elements per lane, 8 per lane, a partly idle row
group), one and four levels, own extents equal to / shorter than the canvas in either direction, repeated indices, the
padding mask, fp32 -> bf16 rounding, the refusals, and arena offsets past 2^31 elements."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CANVAS = [(5, 7), (3, 4), (2, 2), (1, 1)]
# own extents per scene: the canvas; shorter in h only; shorter in w only; shorter in both; 1 x 1
OWN = [
    [(5, 7), (3, 4), (2, 2), (1, 1)],
    [(3, 7), (2, 4), (1, 2), (1, 1)],
    [(5, 4), (3, 2), (2, 1), (1, 1)],
    [(4, 5), (2, 3), (1, 1), (1, 1)],
    [(1, 1), (1, 1), (1, 1), (1, 1)],
]
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _table(own, L, gap=3):
    """(N, 1 + 2L) int64 rows and the arena's row count; ``gap`` unused rows between scenes (a wrong row0 shows)."""
    rows, at = [], gap
    for levels in own:
        rows.append([at] + [v for hw in levels[:L] for v in hw])
        at += sum(h * w for h, w in levels[:L]) + gap
    return torch.tensor(rows, dtype=torch.int64), at


def _reference(arena, table_h, idx, canvas, mask, out_dtype):
    B, C, S = len(idx), arena.shape[1], sum(h * w for h, w in canvas)
    out = torch.zeros((B, S, C), dtype=out_dtype, device=arena.device)
    for b, i in enumerate(idx):
        row = [int(v) for v in table_h[i]]
        r, start = row[0], 0
        for l, (H, W) in enumerate(canvas):
            h, w = row[1 + 2 * l], row[2 + 2 * l]
            out[b, start:start + H * W].view(H, W, C)[:h, :w] = arena[r:r + h * w].view(h, w, C).to(out_dtype)
            r += h * w
            start += H * W
    if mask is not None:
        out[mask != 0] = 0
    return out


def _call(arena, table_h, idx, canvas, mask, out_dtype):
    from demf_amd import ops
    dev = arena.device
    B, S = len(idx), sum(h * w for h, w in canvas)
    out = torch.full((B, S, arena.shape[1]), float("nan"), dtype=out_dtype, device=dev)      # an unwritten row shows
    got = ops.assemble_tokens(arena, table_h.to(dev), torch.tensor(idx, dtype=torch.int64, device=dev), canvas, mask,
                              bf16=out_dtype == torch.bfloat16, out=out)
    assert got is out
    return out


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("C", [4, 36, 256])
@pytest.mark.parametrize("out_dt", ["fp32", "bf16"])
@pytest.mark.parametrize("arena_dt", ["fp32", "bf16"])
def test_assemble_equals_torch_placement(arena_dt, out_dt, C, L):
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(C * 10 + L)
    canvas = CANVAS[:L]
    S = sum(h * w for h, w in canvas)
    assert S % 8 and S % 16 and (3 * S) % 8 and (3 * S) % 16          # no whole number of any block's rows
    table_h, rows = _table(OWN, L)
    arena = torch.randn((rows, C), generator=g).to(DT[arena_dt]).to(dev)
    batches = [[i] for i in range(len(OWN))] + [[0, 3, 0], [1, 2, 4], [4, 4, 2]]      # B = 1 and 3, repeats inside
    for idx in batches:
        B = len(idx)
        mask = (torch.rand((B, S), generator=g) < 0.3).to(torch.uint8) * 255
        mask[:, 0] = 1                                                # (0, 0) of level 0: inside every own extent
        mask[:, S - 1] = 0
        mask = mask.to(dev)
        for m in (None, mask):
            want = _reference(arena, table_h, idx, canvas, m, DT[out_dt])
            got = _call(arena, table_h, idx, canvas, m, DT[out_dt])
            assert torch.equal(_bits(got), _bits(want)), (idx, m is not None)
    # without `out`: a fresh tensor of the asked dtype
    from demf_amd import ops
    fresh = ops.assemble_tokens(arena, table_h.to(dev), torch.tensor([2, 2], device=dev), canvas,
                                bf16=out_dt == "bf16")
    assert fresh.dtype == DT[out_dt] and torch.equal(_bits(fresh), _bits(_reference(arena, table_h, [2, 2], canvas, None,
                                                                                  DT[out_dt])))


def test_fp32_to_bf16_rounds_as_torch():
    """Ties to even (down and up), just above / below a tie, a value that rounds up into the next exponent, +-0, the
    largest finite (-> inf), subnormals (ties, -> the smallest normal) and infinities, against ``.to(torch.bfloat16)``."""
    words = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3FFFFFFF, 0xBFFFFFFF, 0x00000000, 0x80000000,
             0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x00008000, 0x00018000, 0x00008001, 0x007FFFFF, 0x807FFFFF,
             0x7F800000, 0xFF800000, 0x3F800000, 0xC0490FDB]
    dev = torch.device("cuda")
    arena = torch.tensor(words, dtype=torch.int64).to(torch.int32).view(torch.float32).view(5, 4).to(dev)
    table_h = torch.tensor([[0, 1, 5]], dtype=torch.int64)
    got = _call(arena, table_h, [0], [(1, 5)], None, torch.bfloat16)
    want = arena.to(torch.bfloat16).view(1, 5, 4)
    assert torch.equal(_bits(got), _bits(want)), (_bits(got).flatten().tolist(), _bits(want).flatten().tolist())
    # and bf16 -> fp32 is exact
    back = _call(want.view(5, 4).contiguous(), table_h, [0], [(1, 5)], None, torch.float32)
    assert torch.equal(_bits(back), _bits(want.float()))


def test_refusals_launch_nothing():
    from demf_amd import ops
    dev = torch.device("cuda")
    table_h, rows = _table(OWN, 4)
    arena = torch.randn((rows, 8), device=dev)
    S = sum(h * w for h, w in CANVAS)
    table, nan = table_h.to(dev), float("nan")

    def refused(exc, arena, table, idx, canvas, out, **kw):
        with pytest.raises(exc):
            ops.assemble_tokens(arena, table, torch.tensor(idx, dtype=torch.int64, device=dev), canvas, out=out, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), "a refused call wrote into `out`"

    out = torch.full((1, S, 8), nan, device=dev)
    small = [(4, 7)] + CANVAS[1:]                                      # scene 0 is 5 x 7 there
    refused(RuntimeError, arena, table, [0], small, torch.full((1, sum(h * w for h, w in small), 8), nan, device=dev))
    refused(RuntimeError, arena, table, [len(OWN)], CANVAS, out)       # an index outside the table
    refused(RuntimeError, arena, table, [-1], CANVAS, out)
    refused(RuntimeError, torch.randn((rows, 6), device=dev), table, [1], CANVAS, torch.full((1, S, 6), nan, device=dev))
    nine = [(1, 1)] * 9
    t9 = torch.tensor([[0] + [1, 1] * 9], dtype=torch.int64, device=dev)
    refused(RuntimeError, arena, t9, [0], nine, torch.full((1, 9, 8), nan, device=dev))
    refused(ValueError, arena, table, [1], CANVAS, torch.full((1, S + 1, 8), nan, device=dev))       # wrong shape
    refused(ValueError, arena, table, [1], CANVAS, torch.full((1, S, 8), nan, device=dev, dtype=torch.bfloat16))
    refused(ValueError, arena, table, [1], CANVAS, torch.full((1, S, 8), nan, device=dev), bf16=True)
    # a scene whose rows run past the arena's end
    far = table_h.clone()
    far[0, 0] = rows - 3
    refused(RuntimeError, arena, far.to(dev), [0], CANVAS, out)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.assemble_tokens(arena.cpu(), table_h, torch.tensor([0]), CANVAS)


def test_offsets_past_two_to_the_31_elements():
    """A bf16 arena of 2^31 / C + 64 rows at C = 256 (4.3 GB, never filled) with one scene in its last 35 rows: the
    element offsets lie past 2^31, where a 32-bit offset would read another place of the same allocation."""
    dev = torch.device("cuda")
    if torch.cuda.mem_get_info(dev)[0] < 8 << 30:
        pytest.skip("less than 8 GB of device memory free")
    C = 256
    rows = 2 ** 31 // C + 64
    arena = torch.empty((rows, C), dtype=torch.bfloat16, device=dev)
    g = torch.Generator(device="cpu").manual_seed(7)
    arena[rows - 35:] = torch.randn((35, C), generator=g).to(torch.bfloat16).to(dev)
    assert (rows - 35) * C > 2 ** 31
    table_h = torch.tensor([[rows - 35, 5, 7]], dtype=torch.int64)
    for dt in (torch.bfloat16, torch.float32):
        got = _call(arena, table_h, [0, 0], [(5, 7)], None, dt)
        want = arena[rows - 35:].to(dt).view(1, 35, C).expand(2, 35, C)
        assert torch.equal(_bits(got), _bits(want.contiguous()))
