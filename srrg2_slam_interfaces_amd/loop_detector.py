"""Loop-closure candidate drivers on top of the batched aligner: the breadth-first
local-map selector that proposes candidates, the brute-force detector and the relocalizer that align them.

Mirror of MultiLoopDetectorBruteForce_::compute()
(S/registration/loop_detector/multi_loop_detector_brute_force_impl.cpp:12-132): the fixed scene is set ONCE
(:63), every hint is one independent alignment (:64-79) -- here ONE compute_batch() call instead of the
sequential loop -- followed by the accept gates (:80-112) and the closure record (:120-131).
PARAM names and defaults: multi_loop_detector_brute_force.h:20-41.
"""
import numpy as np

from . import _abi as abi
from . import slices as sl


def _set_fixed(al, fixed, fixed_normals):
    """aligner->setFixed(container): one cloud for slice 0, or {slice_idx: cloud} (normals the same form) for every slice
    that reads a cloud of its own"""
    if not isinstance(fixed, dict):
        al.set_fixed(0, fixed, fixed_normals)
        return
    for si in sorted(fixed):
        al.set_fixed(si, fixed[si], fixed_normals.get(si) if isinstance(fixed_normals, dict) else None)


def _align(al, movings, normals, guesses):
    """one batch for the candidates' moving clouds: arrays -> compute_batch (slice 0), {slice_idx: cloud} per candidate ->
    compute_batch_slices (the reference binds the candidate's whole property container, every slice picks its cloud by name:
    multi_loop_detector_brute_force_impl.cpp:63-79, multi_relocalizer_impl.cpp:74-87)"""
    if not any(isinstance(m, dict) for m in movings):
        return al.compute_batch(movings, guesses, normals if all(n is not None for n in normals) else None)
    keys = {tuple(sorted(m)) if isinstance(m, dict) else None for m in movings}
    if len(keys) != 1 or None in keys:
        raise ValueError("per-slice moving clouds: every candidate needs a dict with the same slices")
    slices = sorted(movings[0])
    moving = {si: [m[si] for m in movings] for si in slices}
    moving_normals = {}
    for si in slices:
        per = [n.get(si) if isinstance(n, dict) else None for n in normals]
        moving_normals[si] = per if all(x is not None for x in per) else None
    return al.compute_batch_slices(moving, guesses, moving_normals)


class ClosureHint:
    """LocalMapSelector_::ClosureHint: a candidate local map and the initial guess of moving-in-fixed.  ``moving`` /
    ``moving_normals``: a cloud for slice 0, or {slice_idx: cloud} for an aligner with several cue slices."""

    def __init__(self, local_map_id, moving, moving_normals=None, initial_guess=None):
        self.local_map_id = local_map_id
        self.moving = moving
        self.moving_normals = moving_normals
        self.initial_guess = initial_guess


class MultiLoopDetectorBruteForce:
    def __init__(self, relocalize_aligner, relocalize_min_inliers=500, relocalize_max_chi_inliers=0.005,
                 relocalize_min_inliers_ratio=0.7):
        if relocalize_aligner is None:
            raise RuntimeError("MultiLoopDetectorBruteForce_::compute| no aligner")  # :52-54
        self.relocalize_aligner = relocalize_aligner
        self.relocalize_min_inliers = relocalize_min_inliers
        self.relocalize_max_chi_inliers = relocalize_max_chi_inliers
        self.relocalize_min_inliers_ratio = relocalize_min_inliers_ratio
        self.attempted_closures = []
        self.detected_closures = []
        self.drops = []

    def compute(self, source_local_map_id, fixed, fixed_normals, hints, pose_in_current=None):
        al = self.relocalize_aligner
        dim = al.dim
        pose_in_current = sl.identity(dim) if pose_in_current is None else np.asarray(pose_in_current, np.float32)
        self.attempted_closures = [h.local_map_id for h in hints if h.moving is not None]  # :71-75
        self.detected_closures, self.drops = [], []
        hints = [h for h in hints if h.moving is not None]
        if not hints:
            return self.detected_closures
        _set_fixed(al, fixed, fixed_normals)  # aligner->setFixed(...) once, :63
        guesses = [sl.identity(dim) if h.initial_guess is None else h.initial_guess for h in hints]
        results = _align(al, [h.moving for h in hints], [h.moving_normals for h in hints], guesses)
        for h, r in zip(hints, results):
            if r["status"] != abi.SUCCESS:  # :80-84
                self.drops.append((h.local_map_id, "ALIGNER DROP [code: %d]" % r["status"]))
                continue
            last = r["last"]
            # aligner->numCorrespondences() AFTER compute(), i.e. after _pruneCorrespondences (:89)
            num_correspondences = r.get("num_correspondences", last["num_correspondences"])
            num_inliers = last["num_inliers"]
            chi_inliers = np.float32(last["chi_inliers"]) / np.float32(num_inliers)  # :91
            if num_inliers < self.relocalize_min_inliers:  # :94-97
                self.drops.append((h.local_map_id, "NUM_INLIERS DROP"))
                continue
            if chi_inliers > np.float32(self.relocalize_max_chi_inliers):  # :99-103
                self.drops.append((h.local_map_id, "MAX_CHI_INLIERS DROP"))
                continue
            inlier_ratio = np.float32(num_inliers) / np.float32(num_correspondences)  # :105
            if inlier_ratio < np.float32(self.relocalize_min_inliers_ratio):  # :107-111
                self.drops.append((h.local_map_id, "MIN_INLIERS_RATIO DROP"))
                continue
            X = r["moving_in_fixed"]
            self.detected_closures.append({  # LoopClosure_ ctor arguments, :120-131
                "source": source_local_map_id,
                "target": h.local_map_id,
                "measurement": X,
                "information": np.eye(3 if dim == 2 else 6, dtype=np.float32),
                "pose_in_target": sl.compose(sl.inverse(X), pose_in_current),  # :120
                "chi_inliers": float(chi_inliers),
                "num_inliers": int(num_inliers),
                "num_correspondences": int(num_correspondences),
            })
        return self.detected_closures


class LocalMapSelectorBreadthFirst:
    """LocalMapSelectorBreadthFirst_::compute() (S/registration/local_map_selectors/
    local_map_selector_breadth_first_impl.cpp:12-101): a uniform-cost (hop count) visit of the pose graph from the
    current local map over its enabled factors, then one ClosureHint per local map whose origin lies within a range
    that grows with the graph distance.  PARAM names/defaults: local_map_selector_breadth_first.h:24-48.

    The visit is srrg2_solver's FactorGraphVisit with FactorGraphVisitCostUniform (:52-59; un-vendored): restated as a
    breadth-first search; local maps the visit does not reach are skipped."""

    def __init__(self, relocalize_range_scale=2, aggressive_relocalize_graph_distance=10,
                 aggressive_relocalize_graph_max_range=20, aggressive_relocalize_range_increase_per_edge=0.1,
                 max_local_map_distance=1.0):
        self.relocalize_range_scale = relocalize_range_scale
        self.aggressive_relocalize_graph_distance = aggressive_relocalize_graph_distance
        self.aggressive_relocalize_graph_max_range = aggressive_relocalize_graph_max_range
        self.aggressive_relocalize_range_increase_per_edge = aggressive_relocalize_range_increase_per_edge
        self.max_local_map_distance = max_local_map_distance
        self.hints = []
        self.costs = {}

    def compute(self, estimates, factors, source_id, robot_in_world):
        """estimates: {local map id: pose}; factors: iterable of (i, j, enabled); returns the hints as dicts
        {target, initial_guess (target in source), information, cost}."""
        if source_id not in estimates:
            raise RuntimeError("LocalMapSelectorBreadthFirst_::compute| _current_local_map is NULL")
        adj = {}
        for (i, j, enabled) in factors:
            if not enabled:
                continue
            adj.setdefault(i, []).append(j)
            adj.setdefault(j, []).append(i)
        cost, frontier = {source_id: 0}, [source_id]
        while frontier:
            nxt = []
            for v in frontier:
                for w in adj.get(v, ()):
                    if w not in cost:
                        cost[w] = cost[v] + 1
                        nxt.append(w)
            frontier = nxt
        self.costs = cost
        dim = 2 if np.asarray(robot_in_world).shape == (3, 3) else 3
        world_in_robot = sl.inverse(np.asarray(robot_in_world, np.float32))
        source_inv = sl.inverse(np.asarray(estimates[source_id], np.float32))
        self.hints = []
        for vid in sorted(estimates):  # graph->variables() is ordered by id
            if vid == source_id or vid not in cost:
                continue
            target = np.asarray(estimates[vid], np.float32)
            target_in_robot = sl.compose(world_in_robot, target)  # :69
            guess = sl.compose(source_inv, target)  # :70-71
            c = float(cost[vid])
            range_scale = self.relocalize_range_scale * c * self.aggressive_relocalize_range_increase_per_edge + 1  # :78-80
            range_scale = min(range_scale, float(self.aggressive_relocalize_graph_max_range))
            t = target_in_robot[:2, 2] if dim == 2 else target_in_robot[:, 3]
            if float(np.linalg.norm(t)) > self.max_local_map_distance * range_scale:  # :82-85
                continue
            if c > self.aggressive_relocalize_graph_distance:  # :88-90 aggressive relocalization
                guess = guess.copy()
                if dim == 2:
                    guess[:2, 2] = 0
                else:
                    guess[:, 3] = 0
            self.hints.append({"target": vid, "initial_guess": guess,
                               "information": np.eye(3 if dim == 2 else 6, dtype=np.float32), "cost": c})
        return self.hints


class MultiRelocalizer:
    """MultiRelocalizer_::compute() (S/registration/relocalization/multi_relocalizer_impl.cpp:12-145).  The closure
    candidates come from the loop detector (dicts as MultiLoopDetectorBruteForce.detected_closures plus, for the
    aligner branch, the target local map's cloud).  Without an aligner the best closure is chosen on the detector's
    statistics (:27-66); with one every candidate within max_translation is re-aligned against the current measurement
    -- here in ONE compute_batch() instead of the sequential loop -- gated like the detector (:104-121) and the lowest
    chi per inlier wins (:128-137).  A candidate's ``moving`` / ``moving_normals`` and ``fixed`` / ``fixed_normals`` may be
    {slice_idx: cloud} dicts for an aligner with several cue slices (one compute_batch_slices() then).  PARAMs: multi_relocalizer.h:29-43, relocalizer.h:22."""

    def __init__(self, aligner=None, max_translation=3.0, relocalize_min_inliers=500, relocalize_max_chi_inliers=0.005,
                 relocalize_min_inliers_ratio=0.7):
        self.aligner = aligner
        self.max_translation = max_translation
        self.relocalize_min_inliers = relocalize_min_inliers
        self.relocalize_max_chi_inliers = relocalize_max_chi_inliers
        self.relocalize_min_inliers_ratio = relocalize_min_inliers_ratio
        self.relocalized_closure = None
        self.relocalization_map = None
        self.robot_in_local_map = None
        self.drops = []

    @staticmethod
    def _tnorm(T):
        T = np.asarray(T, np.float32)
        return float(np.linalg.norm(T[:2, 2] if T.shape == (3, 3) else T[:, 3]))

    def compute(self, closure_candidates, fixed=None, fixed_normals=None):
        self.relocalized_closure = self.relocalization_map = None
        self.drops = []
        dim = None
        for c in closure_candidates:
            dim = 2 if np.asarray(c["pose_in_target"]).shape == (3, 3) else 3
            break
        self.robot_in_local_map = sl.identity(dim or 3)
        near = []
        for c in closure_candidates:
            if self._tnorm(c["pose_in_target"]) > self.max_translation:  # :38-42, :84-88
                self.drops.append((c["target"], "MAX_TRANSITION DROP"))
                continue
            near.append(c)
        if self.aligner is None:
            best = None
            for c in near:
                if best is not None:
                    if c["chi_inliers"] > best["chi_inliers"]:  # :45-49
                        self.drops.append((c["target"], "HIGH_CHI_INLIERS DROP"))
                        continue
                    if c["num_correspondences"] < best["num_correspondences"]:  # :50-54
                        self.drops.append((c["target"], "LOW_MIN_CORRESPONDENCE DROP"))
                        continue
                best = c
            if best is not None:  # :62-66
                self.relocalized_closure = best
                self.relocalization_map = best["target"]
                self.robot_in_local_map = np.asarray(best["pose_in_target"], np.float32)
            return self.relocalization_map
        if not near:
            return None
        al = self.aligner
        _set_fixed(al, fixed, fixed_normals)  # aligner->setFixed(&tracker->measurementContainer()), :78
        guesses = [sl.inverse(np.asarray(c["pose_in_target"], np.float32)) for c in near]  # :91
        results = _align(al, [c["moving"] for c in near], [c.get("moving_normals") for c in near], guesses)
        best_chi_average = np.float32(np.finfo(np.float32).max)
        for c, r in zip(near, results):
            if r["status"] != abi.SUCCESS:  # :93-97
                self.drops.append((c["target"], "ALIGNER DROP [code: %d]" % r["status"]))
                continue
            last = r["last"]
            # numCorrespondences() after compute(), i.e. after pruning (multi_relocalizer_impl.cpp:101)
            num_inliers, num_correspondences = last["num_inliers"], r.get("num_correspondences", last["num_correspondences"])
            chi_inliers = np.float32(last["chi_inliers"]) / np.float32(num_inliers)  # :102
            if num_inliers < self.relocalize_min_inliers:  # :108-111
                self.drops.append((c["target"], "NUM_INLIERS DROP"))
                continue
            if chi_inliers > np.float32(self.relocalize_max_chi_inliers):  # :113-117
                self.drops.append((c["target"], "MAX_CHI_INLIERS DROP"))
                continue
            if np.float32(num_inliers) / np.float32(num_correspondences) < np.float32(self.relocalize_min_inliers_ratio):
                self.drops.append((c["target"], "MIN_INLIERS_RATIO DROP"))  # :119-125
                continue
            if chi_inliers < best_chi_average:  # :131-137
                self.relocalization_map = c["target"]
                self.robot_in_local_map = sl.inverse(r["moving_in_fixed"])
                best_chi_average = chi_inliers
                self.relocalized_closure = c
        return self.relocalization_map


class MultiLoopDetectorHBST:
    """MultiLoopDetectorHBST_ (S/registration/loop_detector/multi_loop_detector_hbst_impl.cpp).

    The matching half -- ``addPreviousQuery`` (:41-70) and ``computeCorrespondences`` (:72-197) -- runs on a
    ``descriptors.DescriptorDatabase``: exact, exhaustive matching of 256-bit descriptors on the GPU.  It is the HBST of
    the reference with a single leaf: ``maximum_leaf_size``, ``maximum_partitioning`` and ``maximum_depth`` are accepted
    under their reference names and have no effect, and descriptor merging (``maximum_distance_for_merge``, compiled out
    of the reference by default: ``#ifdef SRRG_MERGE_DESCRIPTORS``, :96-98) is unsupported.  Because a tree search is
    approximate and this one is not, the closures found can be a SUPERSET of what the reference's tree finds.

    The alignment half -- ``_computeAlignments`` (:257-377): per reference local map with enough descriptor matches, a
    one-variable Gauss-Newton solve with the matches kept locked, starting from the identity -- and the accept gates and
    closure record of ``_addLoopClosure`` (:379-447) run all candidates through ONE compute_batch_correspondences().
    ``compute()`` is the two in a row (:12-39); ``compute_alignments`` also takes matches from elsewhere.
    PARAMs: loop_detector.h (relocalize_min_inliers / max_chi_inliers / min_inliers_ratio),
    multi_loop_detector_hbst.h:45-74 (the descriptor ones).  The database is created on ``device`` at the first
    compute_correspondences() unless one is given.

    The query may be a ``mapping.Scene`` that carries descriptors (``Scene.set_features``) in place of the host arrays --
    the local map's cloud the reference reads its descriptors from (:84-85, :131-136).  Then nothing but counts, matches
    and results crosses to the host: the database matches and adds the scene on the device (valid = finite coordinates),
    the detector remembers the scene by graph id, and the alignments bind the scenes' device arrays.  A remembered scene
    must stay alive and unchanged while it can be a candidate, as the reference's local maps do.

    ``consensus`` (not in the reference): None keeps exactly the behaviour above.  A dict of srrg2_consensus_params fields (it
    may be empty: the defaults, untuned) puts a geometric verification in front of the solve: ONE srrg2_consensus_compute
    (``consensus.ConsensusVerifier``) over the candidates that pass the match-count gate; a candidate without a consensus pose or
    with fewer than relocalize_min_inliers inliers is dropped as "CONSENSUS DROP [code: n]" (n: srrg2_consensus_status), the rest
    go through the same ONE batched locked solve, from the consensus poses and on the inlier lists.  The exhaustive matcher
    returns more wrong matches than a tree would, and the robustifier alone does not survive a majority of them from the
    identity.  relocalize_min_inliers_ratio is still taken against the ORIGINAL match count (``num_matches`` of the closure
    record): the verification loosens no gate."""

    def __init__(self, relocalize_aligner, relocalize_min_inliers=500, relocalize_max_chi_inliers=0.005,
                 relocalize_min_inliers_ratio=0.7, maximum_descriptor_distance=25.0, maximum_leaf_size=100,
                 maximum_partitioning=0.1, maximum_depth=16, maximum_distance_for_merge=0.0,
                 minimum_age_difference_to_candidates=0, database=None, device=0, consensus=None):
        if relocalize_aligner is None:
            raise RuntimeError("MultiLoopDetectorHBST::computeAlignments|ERROR: aligner not set")  # :264-268
        if maximum_distance_for_merge != 0:
            raise NotImplementedError("MultiLoopDetectorHBST: maximum_distance_for_merge != 0 is unsupported "
                                      "(descriptor merging is not implemented)")
        from .descriptors import check_match_args

        check_match_args(maximum_descriptor_distance, minimum_age_difference_to_candidates, 0)
        self.relocalize_aligner = relocalize_aligner
        self.relocalize_min_inliers = relocalize_min_inliers
        self.relocalize_max_chi_inliers = relocalize_max_chi_inliers
        self.relocalize_min_inliers_ratio = relocalize_min_inliers_ratio
        self.maximum_descriptor_distance = maximum_descriptor_distance
        self.maximum_leaf_size = maximum_leaf_size  # (no effect: one leaf)
        self.maximum_partitioning = maximum_partitioning  # (no effect)
        self.maximum_depth = maximum_depth  # (no effect)
        self.maximum_distance_for_merge = maximum_distance_for_merge
        self.minimum_age_difference_to_candidates = minimum_age_difference_to_candidates
        self.database = database
        self.device = device
        self.consensus = None if consensus is None else dict(consensus)
        self._verifier = None
        self.last_consensus = None  # the ConsensusVerifier results of the last compute_alignments(), per verified candidate
        self.detected_closures = []
        self.drops = []
        self._graph_id_to_database_index = {}
        self._local_maps_in_database = []  # per database index: (graph id, points, normals)
        self._query = None  # the last query local map: (graph id, descriptors, valid, points, normals)
        self._indices = []
        self._correspondences_per_reference = {}
        self.last_match = None

    def indices(self):
        """database indices of the candidates of the last compute_correspondences(), ascending"""
        return list(self._indices)

    def correspondences(self, index):
        """the correspondences (fixed_idx = query point, moving_idx = reference point, response = distance) of candidate
        ``index`` (a database index)"""
        return self._correspondences_per_reference[index]

    def graph_id(self, index):
        return self._local_maps_in_database[index][0]

    @staticmethod
    def _is_scene(x):
        from .mapping import Scene

        return isinstance(x, Scene)

    def _database(self):
        if self.database is None:
            from .descriptors import DescriptorDatabase

            self.database = DescriptorDatabase(device=self.device)
        return self.database

    def _correspondences_from_scene(self, graph_id, scene):
        self._indices, self._correspondences_per_reference, self.last_match = [], {}, None
        if scene.size() == 0:  # :86-91
            self._query = None
            return self.indices()
        self._query = (graph_id, scene, None, scene, None)
        query_index = self._graph_id_to_database_index.get(graph_id, len(self._local_maps_in_database))
        res = self._database().match_scene(scene, query_index, self.maximum_descriptor_distance,
                                           self.minimum_age_difference_to_candidates, self.relocalize_min_inliers)
        self.last_match = res
        self._indices = [int(r) for r in res.indices]
        self._correspondences_per_reference = {int(r): c for r, c in zip(res.indices, res.correspondences)}
        return self.indices()

    def compute_correspondences(self, graph_id, descriptors, valid=None, points=None, normals=None):
        """computeCorrespondences (:72-161) for the query local map ``graph_id``; points / normals are kept for a later
        add_previous_query() (the reference map's cloud of future alignments).  ``descriptors`` may be a Scene with
        descriptors: it is the whole query (valid, points and normals are its own).  Returns indices()."""
        from .descriptors import as_descriptors, as_valid

        if self._is_scene(descriptors):
            if valid is not None or points is not None or normals is not None:
                raise ValueError("a Scene is the whole query: valid / points / normals come from it")
            return self._correspondences_from_scene(graph_id, descriptors)
        d = as_descriptors(descriptors)
        v = as_valid(valid, len(d))
        self._indices, self._correspondences_per_reference, self.last_match = [], {}, None
        if len(d) == 0:  # :86-91 (an empty query is not added either)
            self._query = None
            return self.indices()
        self._query = (graph_id, d, v, points, normals)
        if self.database is None:
            from .descriptors import DescriptorDatabase

            self.database = DescriptorDatabase(device=self.device)
        # the query index: the database size for a new local map, its own index for a registered one (:117-128)
        query_index = self._graph_id_to_database_index.get(graph_id, len(self._local_maps_in_database))
        res = self.database.match(d, v, query_index, self.maximum_descriptor_distance,
                                  self.minimum_age_difference_to_candidates, self.relocalize_min_inliers)
        self.last_match = res
        self._indices = [int(r) for r in res.indices]
        self._correspondences_per_reference = {int(r): c for r, c in zip(res.indices, res.correspondences)}
        return self.indices()

    def add_previous_query(self):
        """addPreviousQuery (:41-70): the last query local map enters the database unless it is registered already or
        has no valid descriptor."""
        if self._query is None:
            return -1
        graph_id, d, v, points, normals = self._query
        if graph_id in self._graph_id_to_database_index:
            return -1
        index = self.database.add_scene(d) if self._is_scene(d) else self.database.add(d, v)
        if index < 0:
            return -1
        assert index == len(self._local_maps_in_database)
        self._graph_id_to_database_index[graph_id] = index
        self._local_maps_in_database.append((graph_id, points, normals))
        self._query = None
        return index

    def compute(self, graph_id, points, normals=None, descriptors=None, valid=None, pose_in_query=None):
        """compute() (:12-39): computeCorrespondences, then the alignments of the candidates.  The fixed cloud is the
        query local map's points, the moving cloud the reference map's (:333-334); a closure's target is the reference
        map's graph id.  ``points`` may be a Scene with descriptors (then normals / descriptors / valid stay None)."""
        if self._is_scene(points):
            if normals is not None or descriptors is not None or valid is not None:
                raise ValueError("a Scene is the whole query: normals / descriptors / valid come from it")
            self.compute_correspondences(graph_id, points)
        else:
            if descriptors is None:
                raise ValueError("compute: descriptors missing")
            self.compute_correspondences(graph_id, descriptors, valid, points, normals)
        candidates = []
        for r in self._indices:
            gid, ref_points, ref_normals = self._local_maps_in_database[r]
            candidates.append({"reference": gid, "moving": ref_points, "moving_normals": ref_normals,
                               "correspondences": self._correspondences_per_reference[r]})
        return self.compute_alignments(graph_id, points, normals, candidates, pose_in_query)

    def _verify(self, fixed, todo):
        """the consensus poses of the candidates in ONE call; returns (the candidates that keep going, with their inlier lists as
        ``correspondences`` and the original count as ``num_matches``; their consensus poses)"""
        if self._verifier is None:
            from .consensus import ConsensusVerifier

            self._verifier = ConsensusVerifier(self.relocalize_aligner.dim, self.device)
        params = dict(self.consensus)
        params.setdefault("min_inliers", int(self.relocalize_min_inliers))
        results = self._verifier.compute(fixed, [c["moving"] for c in todo], [c["correspondences"] for c in todo], **params)
        self.last_consensus = results
        kept, guesses = [], []
        for c, r in zip(todo, results):
            if r["status"] != abi.CONSENSUS_FOUND or r["num_inliers"] < self.relocalize_min_inliers:
                code = r["status"] if r["status"] != abi.CONSENSUS_FOUND else abi.CONSENSUS_TOO_FEW_INLIERS
                self.drops.append((c["reference"], "CONSENSUS DROP [code: %d]" % code))
                continue
            kept.append(dict(c, correspondences=r["inliers"], num_matches=len(c["correspondences"])))
            guesses.append(r["moving_in_fixed"])
        return kept, guesses

    def _align_scenes(self, fixed, todo, guesses):
        """the batched locked solve on device-resident clouds: the query scene's arrays are the fixed cloud, the candidates'
        (float4 records, stride 16) are concatenated device to device into one buffer for the call"""
        import ctypes as C

        from . import _capi

        lib = _capi.lib()
        lib.srrg2_amd_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        lib.srrg2_amd_device_malloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        lib.srrg2_amd_device_free.argtypes = [C.c_void_p]
        al = self.relocalize_aligner
        addr = lambda p: C.cast(p, C.c_void_p).value  # noqa: E731
        fp, fn, n = fixed.device_arrays()
        al.set_cloud_device("set_fixed", 0, addr(fp), 16, addr(fn) if fn is not None else None, 16, n)
        arrays = [c["moving"].device_arrays() for c in todo]
        with_normals = all(a[1] is not None for a in arrays)
        offsets = np.zeros(len(todo) + 1, np.int32)
        offsets[1:] = np.cumsum([a[2] for a in arrays])
        total = max(int(offsets[-1]), 1)
        bufs = []
        try:
            for _ in range(2 if with_normals else 1):
                p = C.c_void_p()
                if lib.srrg2_amd_device_malloc(C.c_size_t(16 * total), C.byref(p)):
                    raise RuntimeError("srrg2_amd_device_malloc failed")
                bufs.append(p.value)
            for k, (cp, cn, m) in enumerate(arrays):
                for buf, src in zip(bufs, (cp, cn)):
                    if m and lib.srrg2_amd_memcpy(C.c_void_p(buf + 16 * int(offsets[k])), C.c_void_p(addr(src)),
                                                  C.c_size_t(16 * m), 2, None):
                        raise RuntimeError("srrg2_amd_memcpy (device -> device) failed")
            return al.compute_batch_correspondences_device(
                bufs[0], 16, bufs[1] if with_normals else None, 16, offsets, [c["correspondences"] for c in todo],
                guesses)
        finally:
            for b in bufs:
                lib.srrg2_amd_device_free(C.c_void_p(b))

    def compute_alignments(self, query_id, fixed, fixed_normals, candidates, pose_in_query=None):
        """candidates: list of dicts {reference, moving, moving_normals or None, correspondences (fixed_idx = query
        point, moving_idx = reference point)}.  With a Scene as ``fixed`` every candidate's ``moving`` must be a Scene too:
        the clouds are bound from their device arrays."""
        al = self.relocalize_aligner
        dim = al.dim
        pose_in_query = sl.identity(dim) if pose_in_query is None else np.asarray(pose_in_query, np.float32)
        self.detected_closures, self.drops = [], []
        todo = []
        for c in candidates:
            if len(c["correspondences"]) < self.relocalize_min_inliers:  # :309-314
                self.drops.append((c["reference"], "ALIGNER DROP [code: %d]" % abi.NOT_ENOUGH_CORRESPONDENCES))
                continue
            todo.append(c)
        if not todo:
            return self.detected_closures
        scenes = self._is_scene(fixed) or any(self._is_scene(c["moving"]) for c in todo)
        if scenes and not (self._is_scene(fixed) and all(self._is_scene(c["moving"]) for c in todo)):
            raise ValueError("compute_alignments: scenes and host arrays cannot be mixed")
        guesses = [sl.identity(dim)] * len(todo)  # :335
        self.last_consensus = None
        if self.consensus is not None:
            todo, guesses = self._verify(fixed, todo)
            if not todo:
                return self.detected_closures
        if scenes:
            results = self._align_scenes(fixed, todo, guesses)
        else:
            al.set_fixed(0, fixed, fixed_normals)
            normals = [c.get("moving_normals") for c in todo]
            results = al.compute_batch_correspondences(
                [c["moving"] for c in todo], [c["correspondences"] for c in todo], guesses,
                normals if all(n is not None for n in normals) else None)
        for c, r in zip(todo, results):
            if r["status"] != abi.SUCCESS:  # :346-356
                self.drops.append((c["reference"], "ALIGNER DROP [code: %d]" % r["status"]))
                continue
            last = r["last"]
            num_inliers = last["num_inliers"]
            num_correspondences = num_inliers + last["num_outliers"] + last["num_suppressed"]  # :388-389
            chi_inliers = np.float32(last["chi_inliers"]) / np.float32(num_inliers)
            if num_inliers < self.relocalize_min_inliers:  # :394-398
                self.drops.append((c["reference"], "NUM_INLIERS DROP"))
                continue
            if chi_inliers > np.float32(self.relocalize_max_chi_inliers):  # :400-404
                self.drops.append((c["reference"], "MAX_CHI_INLIERS DROP"))
                continue
            # (behind a consensus verification the ratio is still taken against the ORIGINAL match count)
            num_matches = int(c.get("num_matches", len(c["correspondences"])))
            ratio_base = num_matches if self.consensus is not None else num_correspondences
            if np.float32(num_inliers) / np.float32(ratio_base) < np.float32(self.relocalize_min_inliers_ratio):
                self.drops.append((c["reference"], "MIN_INLIERS_RATIO DROP"))  # :406-413
                continue
            reference_in_query = r["moving_in_fixed"]
            D = 3 if dim == 2 else 6
            info = np.eye(D, dtype=np.float32)
            info[dim - 1, dim - 1] = 1e-3  # :429-430 (reduced weight along the last translation axis)
            self.detected_closures.append({
                "source": query_id, "target": c["reference"], "measurement": reference_in_query, "information": info,
                "pose_in_target": sl.compose(sl.inverse(reference_in_query), pose_in_query),  # :420
                "chi_inliers": float(chi_inliers), "num_inliers": int(num_inliers),
                "num_correspondences": int(num_correspondences), "correspondences": c["correspondences"],
                "num_matches": num_matches})
        return self.detected_closures
