"""bench.py --dump-outputs on the host side: the point it writes is float64 and holds the 256-bit coordinates exactly
(16-bit limbs)."""
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _from_limbs(limbs):
    return sum(int(v) << (16 * i) for i, v in enumerate(limbs))


def test_point_round_trips_exactly(tmp_path):
    x, y = (1 << 254) - 189, 0xDEADBEEF << 200
    p = SimpleNamespace(xy=x.to_bytes(32, "little") + y.to_bytes(32, "little"), is_inf=False)
    bench.dump_outputs(str(tmp_path), bench.point_arrays("msm", p))
    xy = np.load(tmp_path / "msm_xy.npy")
    inf = np.load(tmp_path / "msm_is_inf.npy")
    assert xy.dtype == np.float64 and xy.shape == (2, 16)
    assert (_from_limbs(xy[0]), _from_limbs(xy[1])) == (x, y)
    assert inf.tolist() == [0.0]
    ident = bench.point_arrays("msm", SimpleNamespace(xy=bytes(64), is_inf=True))
    assert ident["msm_is_inf"].tolist() == [1.0] and not ident["msm_xy"].any()

