"""Python big-integer model of issuing accumulator witnesses: d = f_V(-y) over all members (vb_accumulator/src/universal.rs:461-495), the scalars of
compute_non_membership_witnesses_for_batch_given_d (:499-535) and of compute_membership_witnesses_for_batch (positive.rs:369-381), and the partition
identity the reference states (:476-478: partition the members, multiply the outputs).
Shared by tests/test_acc_issue_device_code_on_host.py and tests/test_gpu_accumulator_issue.py."""
from acc_model import R


def d_for_batch(members, non_members, d_in=None):
    """d_i = d_in_i prod_j (member_j - y_i); d_in = None: one"""
    out = []
    for i, y in enumerate(non_members):
        d = 1 if d_in is None else d_in[i] % R
        for a in members:
            d = d * (a - y) % R
        out.append(d)
    return out


def d_partitioned(members, non_members, cuts):
    """the same through the partition identity: members cut at `cuts` (sorted positions), every part's output the d_in of the next"""
    d, lo = None, 0
    for hi in list(cuts) + [len(members)]:
        d = d_for_batch(members[lo:hi], non_members, d)
        lo = hi
    return d


def non_membership_scalars(d, non_members, f_v, alpha):
    """(scalar, ok): (f_V - d_i) / (y_i + alpha); a zero d_i (the reference's CannotBeZero) gives (0, False)"""
    out = []
    for di, y in zip(d, non_members):
        assert (y + alpha) % R, "y = -alpha has no inverse"
        out.append((0, False) if di % R == 0 else ((f_v - di) * pow(y + alpha, R - 2, R) % R, True))
    return out


def membership_scalars(members, alpha):
    """1 / (y_i + alpha)"""
    return [pow(y + alpha, R - 2, R) for y in members]
