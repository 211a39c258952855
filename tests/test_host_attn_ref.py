"""tests/attn_ref.py checked on the host: the float64 references against torch autograd and F.scaled_dot_product_attention, the NumPy e4m3
rounding against torch.float8_e4m3fn, every fp32 restatement of the kernels' rounding points inside every bound at every case of the table
(the bounds are attainable by a correct implementation), and every mutant of a restatement caught by the checks
tests/test_gpu_attn_conformance.py runs on the kernels (attn_ref.check_case - the same functions, so "caught here" is "caught there").

Worst ratio to the bound of the unmutated restatements, smallest .. largest over the cases (printed as RANGE with -s):
  bf16 forward     o 0.13 .. 0.82      stored P 0.90 .. 0.99
  fp8 forward      o 0.13 .. 0.52      stored P 0.01 .. 0.62 (the bound carries the e4m3 matrix core's term, which exact fp32 does not use)
  backward         dq 0.15 .. 0.85     dk 0.15 .. 0.89     dv 0.00 .. 0.92     (on the bf16 and on the fp8 forward's o)
  gather backward  dq, dk 0.01 .. 0.03 (the fp32 terms alone)                  dv 0.00 .. 0.48 (many-to-one maps; 0 for permutations: exact)
  three-kernel     dq 0.09 .. 0.66     dk 0.09 .. 0.71     dv 0.09 .. 0.62
The mutants, the first case of attn_ref.CASES order (gather, uniform, bounds) that catches each, and - a record, not an assertion - whether
the whole-tensor bars of tests/test_gpu_ops.py (1e-2 bf16; 1e-1 max-norm and 8e-2 L2 fp8; on those tests' inputs) would have let it pass:
  mutant         caught at                          old bars let it pass: bf16 fwd / fp8 fwd / bf16 bwd
  max_half       gather-B2-N64-perm16 (overflow)    yes / yes / yes     row maximum over one half of the keys only (a missing halves_swap32)
  sum_half       gather-B2-N64-perm16               no  / no  / yes     row sum over one half of the keys only
  d_half         gather-B2-N64-perm16               yes / yes / no      D over 64 of the 128 channels
  d_2pct         gather-B2-N64-perm16               yes / yes / yes     D wrong by 2 %
  ln_lse         bounds-B1-N64-randn0.5             yes / yes / no      natural-log LSE fed to exp2
  no_scale       gather-B2-N64-perm16               yes / yes / no      scale missing from dS
  scale_twice    gather-B2-N64-perm16               yes / yes / no      scale applied twice to dS
  drop_block     gather-B2-N256-perm16              no  / no  / yes     the last 32-key block dropped at N = 256 only
  fp8_vperm      gather-B2-N64-perm16               yes / no  / yes     fp8 V^T key permutation with g and hh not exchanged
  p_order        gather-B2-N64-perm16               no  / no  / yes     stored P's 8 g + 4 h key order with g and h exchanged
  v_xor          gather-B2-N64-perm16               no  / yes / yes     one wrong V-image XOR term (rows with (row & 3) == 1 read the next chunk)
  swap_stats     gather-B2-N64-perm16               yes / yes / no      LSE and D columns exchanged in the stats lookup
  fp8_qk_group   bounds-B1-N64-randn0.5             yes / no  / yes     one of the eight 16-channel groups left out of the fp8 QK^T
  last_query     gather-B2-N64-perm16               yes / yes / no      the last query left out of dK and dV
("yes" under a column the mutant does not touch is trivial; the rows to read are max_half and d_2pct, which every old bar lets pass, and
the layout mutants, which the old bars catch only because their random inputs happen to be dense.)  Wall time of the module: 7 s.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

RANGES = {}


@pytest.fixture(scope="module", autouse=True)
def _ranges():
    yield
    for k in sorted(RANGES):
        print(f"\nRANGE restatement {k}: {RANGES[k][0]:.2f} .. {RANGES[k][1]:.2f}", end="")
    print()


def note(log):
    for k, v in log:
        lo, hi = RANGES.get(k, (v, v))
        RANGES[k] = (min(lo, v), max(hi, v))


@pytest.mark.parametrize("N,sig", [(64, 1.0), (256, 3.0)])
def test_references_agree_with_autograd_and_sdpa(N, sig):
    g = torch.Generator().manual_seed(N)
    qkv = (torch.randn((2, N, 3 * R.C), generator=g, dtype=torch.float64) * sig).requires_grad_(True)
    do = torch.randn((2, N, R.C), generator=g, dtype=torch.float64)
    q, k, v = R.split(qkv)
    o_t = F.scaled_dot_product_attention(q, k, v)              # default scale: 1 / sqrt(C)
    o, P = R.attention_fwd(qkv)
    assert float((o - o_t.detach()).abs().max() / o_t.detach().abs().max()) < 1e-12
    assert float((P.sum(-1) - 1).abs().max()) < 1e-12
    o_t.backward(do)
    for name, a, b in zip("qkv", R.split(R.attention_bwd(qkv, o, do)), R.split(qkv.grad)):
        assert float((a - b).abs().max() / b.abs().max()) < 1e-12, name
    for name, a, b in zip("qkv", R.split(R.attention_bwd(qkv, None, do)), R.split(qkv.grad)):
        assert float((a - b).abs().max() / b.abs().max()) < 1e-12, name


def test_building_block_references():
    g = torch.Generator().manual_seed(1)
    A, B = torch.randn((2, 5, 24), generator=g), torch.randn((2, 7, 24), generator=g)
    assert torch.allclose(R.bgemm_nt(A, B, 0.5), 0.5 * torch.einsum("bmk,bnk->bmn", A.double(), B.double()), rtol=0, atol=1e-13)
    S = (torch.randn((5, 65), generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    dP = torch.randn((5, 65), generator=g, dtype=torch.float64)
    P = torch.softmax(0.25 * S, -1)
    assert torch.allclose(R.softmax_fwd(S, 0.25), P, rtol=0, atol=1e-14)
    P.backward(dP)
    assert float((R.softmax_bwd(P.detach(), dP, 0.25) - S.grad).abs().max()) < 1e-12
    assert torch.equal(R.transpose(A), A.permute(0, 2, 1))


def test_e4m3_rounding_against_torch():
    """every representable magnitude up to 448, every midpoint between two neighbours and the doubles next to it, either sign"""
    grid = torch.arange(0, 127, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
    assert float(grid[-1]) == 448.0 and float(grid[1]) == 2.0 ** -9 and bool((grid[1:] > grid[:-1]).all())
    mid = (grid[1:] + grid[:-1]) / 2
    pts = torch.cat([grid, mid, torch.nextafter(mid, mid * 2), torch.nextafter(mid, mid * 0), grid[1:] * (1 + 2.0 ** -30)])
    pts = torch.cat([pts, -pts]).float()                    # what the conversion sees is an fp32 (bf16 operands, fp32 p)
    want = pts.to(torch.float8_e4m3fn).double()
    for sat in (True, False):
        got = torch.from_numpy(R.e4m3(pts.double().numpy(), saturate=sat))
        assert torch.equal(got, want), (sat, pts[(got != want)][:8])
    assert np.array_equal(R.e4m3(grid.numpy()), grid.numpy())
    # above 448: torch gives 448 up to the tie at 464 and NaN beyond; the contract saturates
    assert R.e4m3(np.array([460.0, 464.0]), saturate=False).tolist() == [448.0, 448.0] and np.isnan(R.e4m3(np.array([500.0]), saturate=False))[0]
    assert float(torch.tensor(460.0).to(torch.float8_e4m3fn).float()) == 448.0 and bool(torch.tensor(500.0).to(torch.float8_e4m3fn).float().isnan())
    assert R.e4m3(np.array([460.0, 480.0, 1024.0, -2048.0, np.inf])).tolist() == [448.0, 448.0, 448.0, -448.0, 448.0]


def test_case_table():
    ids = [R.ident(c) for c in R.CASES]
    assert len(set(ids)) == len(ids)
    for c in R.CASES:
        assert c.B <= 7 and c.N in (64, 128, 256)
        qkv, do = R.make_inputs(c)
        assert qkv.shape == (c.B, c.N, 3 * R.C) and do.shape == (c.B, c.N, R.C) and qkv.dtype == do.dtype == torch.bfloat16
    assert {(c.B, c.N) for c in R.BOUNDS} >= {(B, N) for B in (1, 3, 7) for N in (64, 128, 256)}
    c = R.GATHER[0]
    qkv, _ = R.make_inputs(c)
    q, k, _ = (t.double() for t in R.split(qkv))
    s = q @ k.transpose(1, 2)
    top = s.max(-1).values
    assert bool((top == 2048).all()) and bool(((s == 2048).sum(-1) == 1).all()) and float(s[s != 2048].max()) <= 0


@pytest.mark.parametrize("c", R.CASES, ids=R.ident)
def test_restatement_inside_the_bounds(c):
    log = []
    R.check_case(R.Restated(), c, log)
    if c.family == "bounds" and c.B <= 3:
        qkv, do = R.make_inputs(c)
        R.check_backward(R.Restated(), c, None, log, " three-kernel", qkv=qkv, do=do, three=True)
    note(log)


def _caught(m):
    impl = R.Restated(m)
    for c in R.GATHER + R.UNIFORM + R.BOUNDS:
        try:
            R.check_case(impl, c)
        except AssertionError as e:
            return c, str(e)
    return None, None


@pytest.mark.parametrize("m", sorted(R.MUTANTS))
def test_mutant_is_caught(m):
    c, msg = _caught(m)
    old = R.old_bars(R.Restated(m))
    print(f"\nMUTANT {m:13s} caught at {R.ident(c) if c else '-':32s} old bars pass: " + ", ".join(f"{k} {'yes' if v else 'no'}" for k, v in old.items())
          + f"   [{R.MUTANTS[m]}]", end="")
    assert c is not None, f"{m} ({R.MUTANTS[m]}) passes every check"


def test_max_over_one_half_is_caught_by_overflow():
    """the large-logit (gather) cases: with the maximum of the other half the exponent is +261 and the row is not finite"""
    impl = R.Restated("max_half")
    seen = False
    for c in R.GATHER:
        o, P = impl.fwd(R.make_inputs(c)[0])
        seen |= not bool(torch.isfinite(o.float()).all())
        with pytest.raises(AssertionError):
            R.check_gather_case(impl, c, False)
    assert seen


def test_old_bars_pass_the_unmutated_restatement():
    assert all(R.old_bars(R.Restated()).values())
