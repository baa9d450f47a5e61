"""Test infrastructure: a numpy restatement of the matching half of MultiLoopDetectorHBST_
(S/registration/loop_detector/multi_loop_detector_hbst_impl.cpp:41-197) with the HBST reduced to one leaf, written
from the semantics in DESIGN.md section 5 "Descriptor matching".  The package never imports it.

  add    (:41-70)   only valid descriptors enter; a map with none is not added; the database index is the map count
  match  (:117-161) age gate with the reference's unsigned arithmetic, strict count gate on the pairs before
                    deduplication, (:168-197) per reference descriptor the query of smallest distance, the smallest query
                    point index on a tie; candidates ascending, correspondences ascending in moving_idx.
"""
import numpy as np

CORR = np.dtype([("fixed_idx", np.int32), ("moving_idx", np.int32), ("response", np.float32)])


def random_descriptors(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip_bits(rng, d, k):
    """copy of descriptor row d (32 bytes) with exactly k distinct bits flipped"""
    out = d.copy()
    bits = rng.choice(256, size=k, replace=False)
    for b in bits:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def hamming(Q, D):
    """(len(Q), len(D)) int32 Hamming distances of 256-bit rows"""
    q = np.ascontiguousarray(Q, np.uint8).view(np.uint64).reshape(len(Q), 4)
    d = np.ascontiguousarray(D, np.uint8).view(np.uint64).reshape(len(D), 4)
    out = np.zeros((len(Q), len(D)), np.int32)
    for k in range(4):
        out += np.bitwise_count(q[:, None, k] ^ d[None, :, k]).astype(np.int32)
    return out


def age_gate_passes(query_index, reference_index, min_age):
    """std::fabs(index_query - entry.first) > minimum_age_difference_to_candidates (:150-151), both indices unsigned
    64-bit: the difference wraps for a reference newer than the query"""
    diff = (int(query_index) - int(reference_index)) % (1 << 64)
    return abs(float(diff)) > float(min_age)


class RestatedDatabase:
    def __init__(self):
        self.maps = []  # (valid descriptors, their point indices)

    def add(self, descriptors, valid=None):
        d = np.asarray(descriptors, np.uint8).reshape(-1, 32)
        idx = np.arange(len(d), dtype=np.int32) if valid is None else np.nonzero(np.asarray(valid))[0].astype(np.int32)
        if len(idx) == 0:
            return -1
        self.maps.append((d[idx], idx))
        return len(self.maps) - 1

    def match(self, descriptors, valid=None, query_index=None, max_distance=25.0, min_age=0, min_matches=0,
              only_maps=None):
        """returns dict(indices, num_matches, correspondences (list), map_counts (-1: age gate)); only_maps restricts
        the search to those database indices (every map is independent: a sample of maps gives their exact rows)"""
        d = np.asarray(descriptors, np.uint8).reshape(-1, 32)
        qidx = np.arange(len(d), dtype=np.int32) if valid is None else np.nonzero(np.asarray(valid))[0].astype(np.int32)
        Q = d[qidx]
        q = len(self.maps) if query_index is None else query_index
        maps = range(len(self.maps)) if only_maps is None else sorted(only_maps)
        out = dict(indices=[], num_matches=[], correspondences=[], map_counts={})
        for r in maps:
            if not age_gate_passes(q, r, min_age):
                out["map_counts"][r] = -1
                continue
            ref, ridx = self.maps[r]
            if len(Q) == 0:
                out["map_counts"][r] = 0
                continue
            dist = self._distances(Q, ref)
            m = dist.astype(np.float64) < float(np.float32(max_distance))  # the float threshold vs the integer distance
            count = int(m.sum())
            out["map_counts"][r] = count
            if count == 0 or not count > min_matches:  # a map without a match is not in the match map at all
                continue
            masked = np.where(m, dist, 1 << 20)
            best = np.argmin(masked, axis=0)  # first minimum = smallest query point index among the closest
            keep = m[best, np.arange(len(ref))]
            c = np.zeros(int(keep.sum()), CORR)
            c["fixed_idx"] = qidx[best[keep]]
            c["moving_idx"] = ridx[keep]
            c["response"] = dist[best[keep], np.nonzero(keep)[0]].astype(np.float32)
            out["indices"].append(r)
            out["num_matches"].append(count)
            out["correspondences"].append(c)
        return out

    @staticmethod
    def _distances(Q, ref, chunk=2048):
        return np.concatenate([hamming(Q[i:i + chunk], ref) for i in range(0, len(Q), chunk)], axis=0)
