"""Mutual exclusion for contested landmarks (slamgpu_set_particle_mutex), restated in numpy for ONE particle: steps 1 and 2 of the
header's contract, nothing of the device's structure (no table of holders, no marks in the label array, no batches).

Inputs: L0[nz] the association's labels (slot >= 0, NEW = -1, DISCARD = -2); nis[nz][nf], nd[nz][nf] the gate values of every
(observation, slot) pair; usable[nf]: the slot was in use before the step, is not retired or dead and the particle holds it;
gate_reject.  Outputs: F[nz] and the five counters (steps, contested, lost, rematched, overturned) of this one particle and step."""
import numpy as np

NEW, DISCARD = -1, -2
COUNTERS = ("steps", "contested", "lost", "rematched", "overturned")


def mutex_model(L0, nis, nd, usable, gate_reject):
    L0 = np.asarray(L0, np.int64)
    nis, nd = np.asarray(nis, np.float64), np.asarray(nd, np.float64)
    usable = np.asarray(usable, bool)
    nz = len(L0)
    F = L0.copy()
    cnt = dict.fromkeys(COUNTERS, 0)
    cnt["steps"] = 1 if nz > 0 else 0
    # 1. contest: claimants in ascending q; a later one displaces the keeper only if its (cls, nd) compares smaller
    holder, losers = {}, []
    for l in sorted(set(int(v) for v in L0 if v >= 0)):
        claim = [q for q in range(nz) if L0[q] == l]
        keep = claim[0]
        for q in claim[1:]:
            ck, cq = (0 if nis[keep, l] < gate_reject else 1), (0 if nis[q, l] < gate_reject else 1)
            if cq < ck or (cq == ck and nd[q, l] < nd[keep, l]):
                keep = q
        holder[l] = keep
        if len(claim) > 1:
            cnt["contested"] += 1
            cnt["lost"] += len(claim) - 1
            cnt["overturned"] += 1 if keep != claim[0] else 0
            losers += [q for q in claim if q != keep]
    # 2. re-match: losers in ascending q; the free candidate with the smallest nd, ties to the lower slot
    for q in sorted(losers):
        best, nbest = -1, np.inf
        for j in range(len(usable)):
            if usable[j] and j not in holder and nis[q, j] < gate_reject and nd[q, j] < nbest:
                best, nbest = j, nd[q, j]
        if best >= 0:
            holder[best] = q
            cnt["rematched"] += 1
        F[q] = best if best >= 0 else DISCARD
    return F, cnt
