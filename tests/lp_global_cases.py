"""Generated fluid-LP cases for the device simplex with its tableau in global memory (csrc/fjsp_lp_global.hip).

Built with tests.lp_cases.make_instance / make_states; none fits the LDS rule of csrc/fjsp_lp_device.hip.  Shared by
tests/test_lp_global_reference.py (CPU: the order-independent row choice beyond 128 rows, the coverage these cases must
keep, the size rule) and tests/test_gpu_lp_global.py (the kernel against the host solver, bit for bit).

Shapes of the reset-time state (rows nr = K + M + precedence rows, columns nc = nx + nr + 2):

    g_rows3  K 70  M  8 R 10 2 machines per op   nr 138 nc  280   a third row group (rows 128-137)
    g_rows4  K 100 M 10 R 10 2 machines per op   nr 200 nc  402   a fourth row group (rows 192-199)
    g_cols9  K 24  M 20 R 12 full eligibility    nr  56 nc  538   9 chunks of 64 columns: one past lp_pivots<8>
    g_wide   K 60  M 20 R 12 full                nr 128 nc 1330   21 chunks: the MPPPO generator's worst case
    g_both   K 66  M 16 R 10 6 machines per op   nr 138 nc  536   beyond 128 rows and 512 columns together

Limit pairs (the kernel takes nr <= 256 and nc <= 1536): l_rows256 / l_rows257 (K 125, M 16, 2 machines per op, R 10 / 9
kinds) and l_cols1536 / l_cols1537 (46 single-operation kinds, M 32, nx 1456 / 1457).
"""
from tests import lp_cases as LC

MAX_ROWS = 256                   # csrc/fjsp_lp_limits.h kLpGlobalRows
MAX_COLUMNS = 1536               # kLpGlobalColumns


def global_bytes(K, M, nx, R):
    """fjsp_lp_global_bytes (csrc/fjsp_lp_global.hip), restated: the scratch slot of the largest tableau an instance can
    need, (2K + M - R) x (nx + 2K + M - R + 2) f64 rounded up to 256 bytes; 0 beyond 256 rows or 1536 columns."""
    nr = K + M + (K - R)
    nc = nx + 1 + nr + 1
    if nr > MAX_ROWS or nc > MAX_COLUMNS:
        return 0
    return (nr * nc * 8 + 255) & ~255


def shape(a):
    """(nr, nc) of the largest tableau of the instance."""
    nr = 2 * a.K + a.M - a.R
    return nr, int((a.p > 0).sum()) + nr + 2


def within_global(a):
    return global_bytes(a.K, a.M, int((a.p > 0).sum()), a.R) > 0


_SPECS = (("g_rows3", 31, dict(Jr=[7] * 10, M=8, per_op=2), 131),
          ("g_rows4", 32, dict(Jr=[10] * 10, M=10, per_op=2), 132),
          ("g_cols9", 33, dict(Jr=[2] * 12, M=20), 133),
          ("g_wide", 34, dict(Jr=[5] * 12, M=20), 134),
          ("g_both", 35, dict(Jr=[8] * 8 + [1] * 2, M=16, per_op=6), 135))


def cases():
    out = []
    for name, seed, kw, state_seed in _SPECS:
        a = LC.make_instance(name, seed, **kw)
        out.append(LC.Case(a, LC.make_states(a, state_seed)))
    return out


def limit_cases():
    """[(case, admitted)]: the pairs on either side of the row limit and of the column limit."""
    specs = (("l_rows256", 41, dict(Jr=[13] * 5 + [12] * 5, M=16, per_op=2), 141, True),
             ("l_rows257", 42, dict(Jr=[14] * 8 + [13], M=16, per_op=2), 142, False),
             ("l_cols1536", 43, dict(Jr=[1] * 46, M=32, nx=1456), 143, True),
             ("l_cols1537", 44, dict(Jr=[1] * 46, M=32, nx=1457), 144, False))
    out = []
    for name, seed, kw, state_seed, admitted in specs:
        a = LC.make_instance(name, seed, **kw)
        out.append((LC.Case(a, LC.make_states(a, state_seed)), admitted))
    return out
