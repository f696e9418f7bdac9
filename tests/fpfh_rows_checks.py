"""NumPy restatement of what compute_fpfh_at_rows has to compute besides the descriptors themselves: WHICH rows need an SPFH.

The descriptor of a row is made of its own hybrid neighbour list, its own SPFH and the SPFH of the rows in that list, so the rows
pass computes an SPFH for the union of the chosen rows' lists (a list holds its own row: the row is at distance 0 from itself) and
reports the size of that union as ``n_spfh``."""
import numpy as np

from oracle import oracle_global as og


def marked_rows(points, rows, radius, max_nn, nbrs=None):
    """Sorted distinct rows of the union of the hybrid neighbour lists (oracle_global.hybrid_neighbours) of ``rows``.  ``nbrs``: the
    lists of every row of ``points`` when the caller has them already."""
    nbrs = og.hybrid_neighbours(points, radius, max_nn) if nbrs is None else nbrs
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    if len(rows) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.unique(np.concatenate([np.asarray(nbrs[r][0], dtype=np.int64) for r in rows]))
