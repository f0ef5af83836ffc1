"""`pytorch3d.ops` as far as the reference uses it: `sample_farthest_points(points [N, P, 3], lengths=None, K=50,
random_start_point=False) -> (selected [N, K, 3], idx [N, K])`, which npcd/data/srn.py:179-188 calls with K=num_points to cut an
object's raw surface cloud down to the points of stage 1.  The semantics are pytorch3d's documented ones; the
`start_idx` argument is an extension."""
from npcd.hip.fps import sample_farthest_points

__all__ = ["sample_farthest_points"]
