"""Training data: device-resident position datasets and the 8 board symmetries.

The reference streams every sample through a single-threaded python generator that reads HDF5,
transforms each plane with numpy and builds float64 batches (supervised_policy_trainer.py:19-45).
Here the whole uint8 dataset is loaded into HBM once (one 48-plane 19x19 position is 17.3 KB:
288 GB holds ~16 M of them), and a batch is (index tensor, transform-id tensor): the HIP
pack-input kernel gathers the rows, applies the dihedral transform and converts to the padded
bf16 layout in one pass (K08); labels are remapped through a precomputed [8, S*S] table.
"""
import numpy as np
import torch

# reference order/names (supervised_policy_trainer.py:76-85)
TRANSFORM_NAMES = ["noop", "rot90", "rot180", "rot270", "fliplr", "flipud", "diag1", "diag2"]

BOARD_TRANSFORMATIONS = {
    "noop": lambda feature: feature,
    "rot90": lambda feature: np.rot90(feature, 1),
    "rot180": lambda feature: np.rot90(feature, 2),
    "rot270": lambda feature: np.rot90(feature, 3),
    "fliplr": lambda feature: np.fliplr(feature),
    "flipud": lambda feature: np.flipud(feature),
    "diag1": lambda feature: np.transpose(feature),
    "diag2": lambda feature: np.fliplr(np.rot90(feature, 1))
}


def transform_ids(names):
    return [TRANSFORM_NAMES.index(n) for n in names]


def label_transform_table(S):
    """table[t, p] = index of the one-hot target after transform t (same map as the planes)."""
    table = np.zeros((8, S * S), dtype=np.int64)
    for t, name in enumerate(TRANSFORM_NAMES):
        for p in range(S * S):
            onehot = np.zeros((S, S))
            onehot[divmod(p, S)] = 1
            q = int(np.argmax(BOARD_TRANSFORMATIONS[name](onehot)))
            table[t, p] = q
    return table


def apply_transform_np(planes, t):
    """(F, S, S) planes -> transformed copy (CPU reference path)."""
    fn = BOARD_TRANSFORMATIONS[TRANSFORM_NAMES[t]]
    return np.stack([fn(p) for p in planes])


def _visits_array(visits, n, S):
    """uint16 [N, S*S] or [N, S*S + 1] (pass last) visit counts, validated."""
    v = np.ascontiguousarray(visits)
    if v.ndim != 2 or v.shape[0] != n or v.shape[1] not in (S * S, S * S + 1):
        raise ValueError("visits must be [%d, %d] or [%d, %d], got %s" %
                         (n, S * S, n, S * S + 1, v.shape))
    if v.dtype != np.uint16:
        if v.size and (v.min() < 0 or v.max() > 65535):
            raise ValueError("visit counts must fit uint16")
        v = v.astype(np.uint16)
    return v


def soft_targets_np(visits, tf, table, classes):
    """Host definition of ops.sl_batch_soft: visit rows [B, CD] -> float32 targets
    [B, classes], normalised over the columns the model has a class for (a stored pass count
    without a pass class is dropped first; a pass class without a stored count gets 0) and
    moved through ``table[tf]``; a zero-sum row stays all zero."""
    v = np.asarray(visits, dtype=np.float64)
    B, CD = v.shape
    P = table.shape[1]
    n = min(CD, classes)
    s = v[:, :n].sum(1, keepdims=True)
    q = np.divide(v[:, :n], s, out=np.zeros((B, n)), where=s > 0)
    Y = np.zeros((B, classes), np.float32)
    rows = np.arange(B)[:, None]
    Y[rows, np.asarray(table)[np.asarray(tf)]] = q[:, :P]
    if n > P:
        Y[:, P] = q[:, P]
    return Y


class DeviceDataset(object):
    """uint8 states [N, F, S, S] + flat action labels [N] resident on ``device``; optionally
    ``visits``: uint16 search visit counts [N, S*S] or [N, S*S + 1] (pass last), the dense policy
    targets of ``--targets visits``, and ``outcomes``: fp32 [N, 1], the game's result for the
    player to move (+1 / -1 / 0; training/search_data.py), the policy-value network's value
    targets."""

    def __init__(self, states, actions, device, board=None, visits=None, outcomes=None):
        states = np.asarray(states)
        self.N, self.F, self.S = states.shape[0], states.shape[1], states.shape[-1]
        acts = np.asarray(actions).astype(np.int64)
        labels = acts[:, 0] * self.S + acts[:, 1] if acts.ndim == 2 else acts
        self.device = torch.device(device)
        self.states = torch.from_numpy(np.ascontiguousarray(states, dtype=np.uint8)).to(
            self.device)
        self.labels = torch.from_numpy(labels).to(self.device)
        self.tf_table = torch.from_numpy(label_transform_table(self.S)).to(self.device)
        self._set_visits(visits)
        self.outcomes = None
        if outcomes is not None:
            o = np.asarray(outcomes, dtype=np.float32).reshape(-1, 1)
            if o.shape[0] != self.N:
                raise ValueError("outcomes must hold %d values, got %d" % (self.N, o.shape[0]))
            self.outcomes = torch.from_numpy(np.ascontiguousarray(o)).to(self.device)

    def _set_visits(self, visits):
        self.visits = None
        if visits is not None:
            self.visits = torch.from_numpy(_visits_array(visits, self.N, self.S)).to(self.device)

    @classmethod
    def from_hdf5(cls, h5file, device):
        visits = h5file["visits"][()] if "visits" in h5file else None
        outcomes = h5file["outcomes"][()] if "outcomes" in h5file else None
        return cls(h5file["states"][()], h5file["actions"][()], device, visits=visits,
                   outcomes=outcomes)

    @classmethod
    def synthetic(cls, n, planes, board, device, seed=0, density=0.35, visits=False,
                  outcomes=False):
        """Random binary planes / uniform labels generated on the device (benchmarks); with
        ``visits`` also visit rows [n, board^2 + 1]: ~40 random classes with counts below 64;
        with ``outcomes`` also random +1 / -1 game results [n, 1]."""
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        ds = cls.__new__(cls)
        ds.N, ds.F, ds.S = n, planes, board
        ds.device = torch.device(device)
        ds.states = (torch.rand((n, planes, board, board), generator=g, device=device) <
                     density).to(torch.uint8)
        ds.labels = torch.randint(0, board * board, (n,), generator=g, device=device)
        ds.tf_table = torch.from_numpy(label_transform_table(board)).to(ds.device)
        ds.visits = None
        if visits:
            C = board * board + 1
            keep = torch.rand((n, C), generator=g, device=device) < 40.0 / C
            counts = torch.randint(1, 64, (n, C), generator=g, device=device)
            counts = counts * keep
            counts[torch.arange(n, device=device), ds.labels] += 64  # the move played leads
            ds.visits = counts.to(torch.int32).to(torch.uint16)
        ds.outcomes = None
        if outcomes:
            ds.outcomes = (torch.randint(0, 2, (n, 1), generator=g, device=device) * 2
                           - 1).float()
        return ds

    def batch_labels(self, index, tf):
        return self.tf_table[tf, self.labels[index]]

    def batch_targets(self, index, tf, classes=None):
        """CPU definition of the visit targets: float32 [B, classes] (numpy)."""
        if self.visits is None:
            raise ValueError("this dataset holds no visits")
        rows = self.visits.cpu().numpy()[index.cpu().numpy()]
        return soft_targets_np(rows, tf.cpu().numpy(), self.tf_table.cpu().numpy(),
                               classes or self.S * self.S)

    def host_states(self, index):
        return self.states.cpu().numpy()[index.cpu().numpy()]

    def host_batch(self, index, tf, soft=False, classes=None):
        """CPU path: (X float32 [B,F,S,S], Y [B,S*S]) materialised with numpy; Y one-hot at the
        transformed label, or with ``soft`` the transformed, normalised visit row ([B, classes],
        classes = S*S by default)."""
        tfs = tf.cpu().numpy()
        X = np.stack([apply_transform_np(s, t) for s, t in
                      zip(self.host_states(index), tfs)]).astype(np.float32)
        if soft:
            return X, self.batch_targets(index, tf, classes)
        lab = self.batch_labels(index.to(self.device), tf.to(self.device)).cpu().numpy()
        Y = np.zeros((len(tfs), self.S * self.S), np.float32)
        Y[np.arange(len(tfs)), lab] = 1
        return X, Y
