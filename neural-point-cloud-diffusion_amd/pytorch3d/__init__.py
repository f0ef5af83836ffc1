"""Drop-in for the one operator of the `pytorch3d` package that the reference imports (npcd/data/srn.py:179):
`from pytorch3d.ops import sample_farthest_points`.  Backed by the gfx950 HIP kernel in libnpcd_hip.so.

This is NOT pytorch3d: it holds nothing else.  Keep it behind a real pytorch3d on sys.path, never ahead of one."""
from . import ops

__all__ = ["ops"]
