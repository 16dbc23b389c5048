"""Selection mode BEST in numpy (include/vitvs.h vitvs_last_order): the statement csrc/select.hip is tested against.

For one frame pair, tables nn_1, nn_2 (ids) and sim_1 (fp32) over the T = g * g tokens of the desired frame:

  class_i = 0 when i is a mutual nearest neighbour (0 <= nn_1[i] < T and nn_2[nn_1[i]] == i), else 1
  cell_i  = ((i // g) * c // g) * c + ((i % g) * c // g),  c = min(cells, g)
  rho_i   = number of tokens k of the same class and cell in front of i: sim_1[k] > sim_1[i], or equal and k < i (fp32 compares)
  order   = the T tokens sorted ascending by (class, rho, -sim_1, id)

The selection is what mode ORDER does with that order: the first num_pairs candidates met (``selected``)."""
import numpy as np


def cells_of(T, cells):
    """Cell id of every token, and c = min(cells, g)."""
    g = int(np.sqrt(T))
    assert g * g == T and 1 <= cells <= 16
    c = min(int(cells), g)
    i = np.arange(T, dtype=np.int64)
    return ((i // g) * c // g) * c + ((i % g) * c // g), c


def mutual_mask(nn_1, nn_2):
    nn_1, nn_2 = np.asarray(nn_1, np.int64), np.asarray(nn_2, np.int64)
    T = nn_1.shape[0]
    ok = (nn_1 >= 0) & (nn_1 < T)
    back = nn_2[np.where(ok, nn_1, 0)]
    return ok & (back == np.arange(T))


def ranks(nn_1, nn_2, sim_1, cells):
    """(class, cell, rho) of every token; rho by the definition, one group at a time."""
    sim = np.asarray(sim_1, np.float32)
    T = sim.shape[0]
    cls = np.where(mutual_mask(nn_1, nn_2), 0, 1).astype(np.int64)
    cell, _ = cells_of(T, cells)
    rho = np.zeros(T, np.int64)
    group = cls * 256 + cell
    for gid in np.unique(group):
        ids = np.nonzero(group == gid)[0]                        # ascending ids
        s = sim[ids]
        before = (s[None, :] > s[:, None]) | ((s[None, :] == s[:, None]) & (ids[None, :] < ids[:, None]))
        rho[ids] = before.sum(axis=1)
    return cls, cell, rho


def best_order(nn_1, nn_2, sim_1, cells=4):
    """The visiting order of one pair: int32 [T], a permutation of 0 .. T-1."""
    sim = np.asarray(sim_1, np.float32)
    cls, _, rho = ranks(nn_1, nn_2, sim, cells)
    ids = np.arange(sim.shape[0])
    # lexsort: the last key is the primary one; -sim of +-0 compares equal, as the fp32 values do
    return np.lexsort((ids, -sim.astype(np.float64), rho, cls)).astype(np.int32)


def selected(nn_1, nn_2, sim_1, num_pairs, cells=4):
    """The tokens mode ORDER keeps on that order: the first num_pairs mutual nearest neighbours met (no same-image shortcut)."""
    order = best_order(nn_1, nn_2, sim_1, cells)
    m = mutual_mask(nn_1, nn_2)
    return order[m[order]][:num_pairs]
