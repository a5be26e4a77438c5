"""Mirror of the reference's ``pkg/controller`` decision path over the GPU path.

* ``calc_percent_usage`` / ``calc_scale_up_delta`` — pkg/controller/util.go:58 / :13
  (the library's bit-exact scalar build of the K4 kernel's arithmetic).
* ``taint_oldest_n`` / ``untaint_newest_n`` — scale_down.go:171 / scale_up.go:118 orderings
  (GPU radix sort; every taint/untaint succeeds, i.e. the dry-mode walk).
* ``Controller`` — (*Controller).RunOnce (controller.go:400) over every group in ONE
  batched decision: listers -> K0 packer -> HIP reduce -> K4 decide.
* ``ResidentController`` — the same RunOnce on the snapshot that stays on the device, fed by
  informer events through ``events.EventQueue`` instead of re-listing and reloading per scan.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

ERRORS = {L.ESC_ST_OK: None, L.ESC_ST_ERR_MIN_NODES: "node count less than the minimum",
          L.ESC_ST_ERR_MAX_NODES: "node count larger than the maximum",
          L.ESC_ST_ERR_DIV_ZERO: "cannot divide by zero in percent calculation",
          L.ESC_ST_ERR_NEG_DELTA: "negative scale up delta",
          L.ESC_ST_ERR_OVERFLOW: "int64 overflow (Quantity inf.Dec regime, not emulated)"}


def calc_percent_usage(cpu_request: int, mem_request: int, cpu_capacity: int, mem_capacity: int,
                       number_of_untainted_nodes: int):
    """calcPercentUsage — pkg/controller/util.go:58.  Returns (cpu%, mem%, error-or-None)."""
    a, b = C.c_double(), C.c_double()
    st = L.load().esc_calc_percent_usage(cpu_request, mem_request, cpu_capacity, mem_capacity,
                                         number_of_untainted_nodes, C.byref(a), C.byref(b))
    return a.value, b.value, ERRORS.get(st, "status %d" % st)


def calc_scale_up_delta(n_untainted: int, cpu_percent: float, mem_percent: float, cpu_request: int,
                        mem_request: int, cached_cpu_m: int, cached_mem_b: int, scale_up_threshold_percent: int):
    """calcScaleUpDelta — pkg/controller/util.go:13.  Returns (delta, error-or-None)."""
    d = C.c_int64()
    st = L.load().esc_calc_scale_up_delta(n_untainted, cpu_percent, mem_percent, cpu_request, mem_request,
                                          cached_cpu_m, cached_mem_b, scale_up_threshold_percent, C.byref(d))
    return d.value, ERRORS.get(st, "status %d" % st)


def _order(created_ns, n: int, oldest: bool, device: int) -> list[int]:
    from .k8s import _device_ctx
    ctx = _device_ctx(device)
    ts = np.ascontiguousarray(created_ns, np.int64)
    k = max(0, min(int(n), len(ts)))
    out = np.zeros(max(k, 1), np.int64)
    L.check(ctx.lib.esc_order_by_creation(ctx.handle, ts.ctypes.data_as(C.POINTER(C.c_int64)), len(ts),
                                          int(oldest), k, out.ctypes.data_as(C.POINTER(C.c_int64))),
            "esc_order_by_creation")
    return [int(x) for x in out[:k]]


def taint_oldest_n(created_ns, n: int, device: int = 0) -> list[int]:
    """taintOldestN — scale_down.go:171: indices (into the given list) of the n oldest."""
    return _order(created_ns, n, True, device)


def untaint_newest_n(created_ns, n: int, device: int = 0) -> list[int]:
    """untaintNewestN — scale_up.go:118: indices of the n newest (over the tainted list)."""
    return _order(created_ns, n, False, device)


# The methods Controller calls on its actuator (per node: taint / untaint return whether the
# API write succeeded; the cloud node group's TargetSize / MaxSize / IncreaseSize /
# DeleteNodes, cloudprovider/interface.go:45-80)
ACTUATOR_METHODS = ("taint", "untaint", "target_size", "max_size", "increase_size", "delete_nodes")


INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
# the decision branches after which scaleNodeGroup reaches calculateNewNodeMetrics
# (controller.go:325): past every early return and the lock
ARMED_BRANCHES = ("fast_down", "slow_down", "scale_up", "none")


def new_node_since(prev_delta: int, branch: str, status: int, last_scale_out) -> int:
    """The `since` word of one group for esc_new_nodes_eval (Context.new_nodes).

    calculateNewNodeMetrics (controller.go:157-189) runs when this scan's scaleNodeGroup gets
    to :325 — its branch is one of ARMED_BRANCHES; empty, gate, below_min, pct_err and locked
    return before — and does its loop only when the previous scan's delta was positive
    (``nodeGroup.scaleDelta > 0``, :165).  `status` takes no part: a scale_up whose
    calcScaleUpDelta fails (ESC_ST_ERR_NEG_DELTA) fails at :346, after :325.  Armed: the
    group's lastScaleOut in Unix ns, INT64_MIN for ``None`` (the zero time.Time: every node is
    newer); unarmed: INT64_MAX (not evaluated)."""
    if int(prev_delta) > 0 and branch in ARMED_BRANCHES:
        return INT64_MIN if last_scale_out is None else int(last_scale_out)
    return INT64_MAX


class SimulatedCloud:
    """The actuator used when none is given: every Kubernetes write succeeds, and the
    cloud node group behaves like the reference tests' mock (pkg/test/cloud_provider.go):
    TargetSize is the group's listed node count and MaxSize its ``max_nodes``;
    IncreaseSize and DeleteNodes succeed."""

    def __init__(self, groups):
        self.groups = groups
        self.size = [0] * len(groups)

    def observe(self, g: int, n_nodes: int):
        self.size[g] = int(n_nodes)

    def taint(self, g: int, node: int) -> bool:
        return True

    def untaint(self, g: int, node: int) -> bool:
        return True

    def target_size(self, g: int) -> int:
        return self.size[g]

    def max_size(self, g: int) -> int:
        return int(self.groups[g].get("max_nodes", 0))

    def increase_size(self, g: int, n: int):
        self.size[g] += n

    def delete_nodes(self, g: int, nodes: list[int]):
        self.size[g] -= len(nodes)


class Controller:
    """RunOnce over every node group as one GPU decision, plus the actuation bookkeeping
    the next run depends on.

    ``list_pods`` / ``list_nodes`` play the informer-backed listers
    (pkg/k8s/pod_listers.go:33, node_listers.go:33): callables returning the full
    cluster lists (plain-dict records, escalator_amd/objects.py) or raising.

    Host state kept across runs, as the reference's NodeGroupState (controller.go:28-44):
      * cached capacity of allNodes[0] (controller.go:207-211);
      * the scale-up lock (scale_lock.go): ScaleUp locks it with the nodes it added
        (scale_up.go:39); while ``clock() - lock_time < scale_up_cool_down_ns`` every run
        returns ``requestedNodes`` (controller.go:317-323), after that it unlocks;
      * the dry-mode taintTracker: taintOldestN appends the names it "taints"
        (scale_down.go:197-200), untaintNewestN deletes the newest tracked names
        (scale_up.go:146-158); filterNodes reads it on the next run (controller.go:126-138).

    Actuation follows the reference's walk: taintOldestN / untaintNewestN go down the GPU
    ordering one node at a time and skip a node whose API write fails until n writes
    succeeded (scale_down.go:179-202, scale_up.go:127-160); the cloud add is clamped to
    MaxSize - TargetSize (calculateNodesToAdd, scale_up.go:48-56) in wet and dry mode, and a
    clamp <= 0 is scaleUpCloudProviderNodeGroup's error without a lock (scale_up.go:66-74);
    TryRemoveTaintedNodes (scale_down.go:51-136) runs before tainting and in the no-change
    branch (controller.go:369-383) on the GPU's reaping pass.  The walks read the selections
    the decision delivers (esc_selections: each group's first n + ``selection_slack`` nodes of
    its order, written to pinned memory inside the step) and continue on esc_group_order only
    when failed writes use up the slack (``walk_fallback`` in the group's result).  The ``actuator`` provides
    ``taint(g, node) -> bool``, ``untaint(g, node) -> bool``, ``target_size(g)``,
    ``max_size(g)``, ``increase_size(g, n)`` and ``delete_nodes(g, nodes)`` (raising on an
    API error); without one a ``SimulatedCloud`` stands in (every write succeeds).

    ``scale_delta[g]`` and ``last_scale_out[g]`` are NodeGroupState's remaining two fields
    (controller.go:38-39): the delta each scan returned, error returns included (:434), and
    ``clock()`` of the scan's ``delta > 0`` arm (:376; ``None`` = the zero time).  They feed
    calculateNewNodeMetrics (controller.go:157-189), which is opt-in: when the actuator has
    ``instantiation_time(g, node) -> int | None`` (Unix ns; ``None`` or raising is GetInstance's
    error, :174), every scan evaluates the armed groups (``new_node_since``) on the device,
    asks the actuator about the nodes listed as unknown, uploads the answers, evaluates again
    if any came, and adds ``r["new_nodes"]`` (n_new, n_observed, n_unknown, lag_sum_ns, buckets,
    expected = the previous delta: the reference warns when it differs from n_observed, :185)
    to the armed groups' records — before the action switch, as the reference does.  Without
    that method nothing is called and no key is added."""

    def __init__(self, groups: list[dict], device: int = 0, dry_mode: bool = False, clock=None, actuator=None,
                 selection_slack: int = 4):
        import time
        from .context import Context
        self.groups = [dict(g, dry_mode=bool(g.get("dry_mode")) or dry_mode) for g in groups]
        self.ctx = Context(self.groups, device=device)
        self.ctx.set_order_in_step(True)                   # the orderings and the walks' prefixes
        self.ctx.set_selections(selection_slack)           # come with every decision
        self._sel = None
        self.state = [{"locked": False, "requested_nodes": 0, "cached_cpu_m": 0, "cached_mem_b": 0}
                      for _ in groups]
        self.lock_time = [None] * len(groups)          # scaleLock.lockTime (None: never locked)
        self.scale_delta = [0] * len(groups)           # NodeGroupState.scaleDelta   controller.go:38, :434
        self.last_scale_out = [None] * len(groups)     # NodeGroupState.lastScaleOut controller.go:39, :376
        self.inst_ns: dict[str, int] = {}              # node name -> instantiation time (Unix ns) learned so far
        self._inst_created: dict[str, int] = {}        # ... and the creation time of the node it was learned for
        self._created: list[int] = []                  # creation times of this scan's listing
        self._new_nodes = None
        self.taint_tracker = {g: [] for g in range(len(groups))}
        self.clock = clock or time.time_ns
        self.actuator = actuator if actuator is not None else SimulatedCloud(self.groups)
        # the actuator protocol (per-node taint/untaint -> bool, the cloud group's sizes):
        # refused here rather than by an AttributeError after a decision
        missing = [m for m in ACTUATOR_METHODS if not callable(getattr(self.actuator, m, None))]
        if missing:
            raise TypeError("actuator %r lacks %s (the protocol: %s; see INTEGRATION.md §5)" %
                            (type(self.actuator).__name__, ", ".join(missing), ", ".join(ACTUATOR_METHODS)))

    def _lock_states(self, now: int):
        """scaleLock.locked() (scale_lock.go:22-29) for every group, before the decision."""
        for g, grp in enumerate(self.groups):
            t = self.lock_time[g]
            if t is not None and now - t < int(grp.get("scale_up_cool_down_ns", 0)):
                self.state[g]["locked"] = True
            else:                                          # unlock(): requestedNodes = 0
                self.state[g]["locked"] = False
                self.state[g]["requested_nodes"] = 0

    def _walk(self, g: int, which: int, n_avail: int, out: dict):
        """The order a taint / untaint walk goes down (0: untainted oldest first, 1: tainted
        newest first): the selection the decision delivered, then — only if the walk needs
        more (failed writes used up the slack, or the list was cut) — esc_group_order beyond it."""
        got = []
        if self._sel is not None:
            w, off, idx = self._sel
            if int(w[g]) >= 0 and int(w[g]) & 3 == which:
                got = [int(j) for j in idx[off[g]:off[g + 1]]]
        yield from got
        if len(got) >= n_avail:                             # the list is the whole order
            return
        out["walk_fallback"] = True
        yield from (int(j) for j in self.ctx.group_order(g, which)[len(got):])

    def _scale_up(self, g: int, n: int, n_tainted: int, names: list[str], out: dict):
        """ScaleUp (scale_up.go:14-46): untaintNewestN over the tainted nodes, the rest
        from the cloud node group (clamped to its MaxSize), then the lock.  Returns
        (nodes brought up, error-or-None)."""
        dry = self.groups[g]["dry_mode"]
        picked = []
        if n_tainted and n > 0:                            # scaleUpUntaint :98-116
            # the count is checked after each pick, so the walk never asks for a node past
            # the last one it needs (that would read on beyond the delivered selection)
            for j in self._walk(g, 1, n_tainted, out):     # newest first (sort.go:27-39), untaintNewestN :127-160
                if dry:                                    # delete the tracked name, if any
                    trk = self.taint_tracker[g]
                    if names[j] in trk:
                        trk.remove(names[j])
                        picked.append(j)
                elif self.actuator.untaint(g, j):          # a failed write moves on
                    picked.append(j)
                if len(picked) >= n:
                    break
        out["untainted_now"] = picked
        rest = n - len(picked)
        out["added"] = 0
        if rest <= 0:
            return len(picked), None
        # scaleUpCloudProviderNodeGroup :58-96 with calculateNodesToAdd :48-56
        target, mx = int(self.actuator.target_size(g)), int(self.actuator.max_size(g))
        add = mx - target if target + rest > mx else rest
        if add <= 0:
            return 0, ("refusing to scaleup up beyond the maximum size of the autoscaling group "
                       "(TargetSize: %d; MaxNodes: %d). Taking no action" % (target, int(self.groups[g].get("max_nodes", 0))))
        if not dry:
            try:
                self.actuator.increase_size(g, add)
            except Exception as e:                         # :84-87
                return 0, str(e)
        self.lock_time[g] = self.clock()                   # scaleLock.lock(added) :39
        self.state[g]["locked"] = True
        self.state[g]["requested_nodes"] = add
        out["added"] = add
        return len(picked) + add, None

    def _scale_down_taint(self, g: int, n: int, n_untainted: int, names: list[str], out: dict):
        """scaleDownTaint -> taintOldestN (scale_down.go:138-205) with the clamped n: the
        untainted nodes oldest first until n taints succeeded."""
        dry = self.groups[g]["dry_mode"]
        picked = []
        for j in (self._walk(g, 0, n_untainted, out) if n > 0 else ()):
            if dry:
                self.taint_tracker[g].append(names[j])
                picked.append(j)
            elif self.actuator.taint(g, j):
                picked.append(j)
            if len(picked) >= n:
                break
        out["tainted_now"] = picked

    def _reap(self, g: int, out: dict):
        """TryRemoveTaintedNodes (scale_down.go:51-136): the GPU pass's toBeDeleted list
        for the group, handed to the cloud node group (DeleteNodes) in wet mode."""
        n = int(self._removal[g]["n_delete"])
        nodes = [int(j) for j in self.ctx.removal_nodes(g)] if n else []
        out["removed"] = nodes
        out["pods_evicted"] = int(self._removal[g]["pods_remaining"]) if n else 0
        if nodes and not self.groups[g]["dry_mode"]:
            try:
                self.actuator.delete_nodes(g, nodes)
            except Exception as e:
                out["reap_err"] = str(e)

    def _learned(self, name: str, j: int, t: int):
        """Keeps an answer in the host's copy of the device's per-node fact: name -> time, and
        beside it the creation time of the node that got the answer (this scan's listing)."""
        self.inst_ns[name] = t
        self._inst_created[name] = self._created[j]

    def _new_node_pass(self, dec, names):
        """calculateNewNodeMetrics (controller.go:157-189) for the groups this decision arms:
        {g: record}, or None when the actuator has no ``instantiation_time``."""
        lookup = getattr(self.actuator, "instantiation_time", None)
        if not callable(lookup):
            return None
        since = [new_node_since(self.scale_delta[g], L.BRANCHES[int(dec[g]["branch"])], int(dec[g]["status"]),
                                self.last_scale_out[g]) for g in range(len(self.groups))]
        armed = [g for g, s in enumerate(since) if s != INT64_MAX]
        if not armed:
            return {}
        rec = self.ctx.new_nodes(since)
        asked, ids, times = set(), [], []
        for g in armed:
            if int(rec[g]["n_new"]) == int(rec[g]["n_observed"]):
                continue
            idx, known = self.ctx.new_nodes_list(g)
            for j in (int(j) for j in idx[known == 0]):
                if j in asked:                             # (a node of two groups: asked once)
                    continue
                asked.add(j)
                try:                                       # GetInstance, controller.go:173
                    t = lookup(g, j)
                except Exception:
                    t = None
                if t is not None:                          # an instance's launch time never changes
                    ids.append(j)
                    times.append(int(t))
                    self._learned(names[j], j, int(t))
        if ids:
            self.ctx.nodes_instantiated(ids, times)
            rec = self.ctx.new_nodes(since)
        return {g: {"n_new": int(rec[g]["n_new"]), "n_observed": int(rec[g]["n_observed"]),
                    "n_unknown": int(rec[g]["n_new"]) - int(rec[g]["n_observed"]),
                    "lag_sum_ns": int(rec[g]["lag_sum_ns"]), "buckets": [int(x) for x in rec[g]["bucket"]],
                    "expected": int(self.scale_delta[g])} for g in armed}

    def _list_error(self, e) -> list[dict]:
        self.scale_delta = [0] * len(self.groups)          # scaleNodeGroup returned 0, err (controller.go:434)
        return [{"delta": 0, "err": str(e)} for _ in self.groups]

    def run_once(self, list_pods, list_nodes) -> list[dict]:
        try:
            pods = list_pods()
        except Exception as e:                   # controller.go:195-198
            return self._list_error(e)
        try:
            nodes = list_nodes()
        except Exception as e:                   # controller.go:202-205
            return self._list_error(e)
        from .objects import placement
        now = self.clock()
        self._lock_states(now)
        trackers = {g: list(t) for g, t in self.taint_tracker.items() if t}
        P, N = self.ctx.pack(pods, nodes, trackers)
        self.ctx.load(P, N)
        tot, dec = self.ctx.decide_all(self.state)       # the ordering is in the step
        try:
            self._sel = self.ctx.selections()
        except L.EscError as e:
            if e.code != L.ESC_E_ORDER:
                raise
            self._sel = None                               # that ordering gave up: order afresh,
            self.ctx.sort_nodes()                          # the walks read esc_group_order
        # CreateNodeNameToInfoMap (controller.go:259) + the reaping pass for every group
        self.ctx.load_placement(*placement(pods, nodes))
        soft = [int(grp.get("soft_delete_grace_ns", 0)) for grp in self.groups]
        hard = [int(grp.get("hard_delete_grace_ns", 0)) for grp in self.groups]
        self._removal = self.ctx.try_remove(now, soft, hard)
        names = [n.get("name", "") for n in nodes]
        if callable(getattr(self.actuator, "instantiation_time", None)):
            # the load left every instantiation time unknown: the ones learned on earlier scans
            # go back in.  A name that is no longer listed is forgotten, and so is one whose
            # node was registered again between two scans (its creation time differs): a node
            # back under a name is a new instance
            index = {m: j for j, m in enumerate(names)}
            self._created = [int(n.get("created_ns", 0)) for n in nodes]
            self.inst_ns = {m: t for m, t in self.inst_ns.items()
                            if m in index and self._inst_created.get(m) == self._created[index[m]]}
            self._inst_created = {m: self._inst_created[m] for m in self.inst_ns}
            if self.inst_ns:
                self.ctx.nodes_instantiated([index[m] for m in self.inst_ns], list(self.inst_ns.values()))
        self._new_nodes = self._new_node_pass(dec, names)
        return self._act(tot, dec, names)

    def _act(self, tot, dec, names) -> list[dict]:
        """The per-group action switch of one scan (controller.go:265-383) over the decision
        `tot` / `dec` and self._sel / self._removal; names[j] = the name of snapshot node j."""
        out = []
        for g in range(len(self.groups)):
            d = dec[g]
            self.state[g]["cached_cpu_m"] = int(d["cached_cpu_m"])        # controller.go:208-211
            self.state[g]["cached_mem_b"] = int(d["cached_mem_b"])
            if hasattr(self.actuator, "observe"):
                self.actuator.observe(g, int(tot["n_nodes"][g]))
            branch = L.BRANCHES[int(d["branch"])]
            r = {"delta": int(d["delta"]), "err": ERRORS.get(int(d["status"])),
                 "branch": branch, "cpu_pct": float(d["cpu_pct"]),
                 "mem_pct": float(d["mem_pct"]), "n_to_taint": int(d["n_to_taint"]),
                 "totals": {k: int(tot[g][k]) for k in tot.dtype.names},
                 "tainted_now": [], "untainted_now": [], "added": 0, "removed": [], "pods_evicted": 0,
                 "walk_fallback": False}
            if self._new_nodes and g in self._new_nodes:                  # controller.go:325
                r["new_nodes"] = self._new_nodes[g]
            n_tainted, n_untainted = int(tot["n_tainted"][g]), int(tot["n_untainted"][g])
            if branch == "below_min":                                     # controller.go:281-295
                r["delta"], r["err"] = self._scale_up(g, r["delta"], n_tainted, names, r)
            elif r["err"] is None and branch in ("fast_down", "slow_down", "scale_up", "none"):
                # the action switch is on nodesDelta's sign, whichever branch computed it
                # (controller.go:367-383; a scale-up from zero can compute 0)
                if r["delta"] < 0:
                    self._reap(g, r)                                      # ScaleDown: reap first
                    if int(d["taint_status"]) == 0:
                        self._scale_down_taint(g, r["n_to_taint"], n_untainted, names, r)   # controller.go:368-371
                    else:
                        r["action_err"] = "taint clamp"                   # scale_down.go:150-154
                elif r["delta"] > 0:
                    _, r["action_err"] = self._scale_up(g, r["delta"], n_tainted, names, r)   # :372-375
                    self.last_scale_out[g] = self.clock()                 # controller.go:376
                else:
                    self._reap(g, r)                                      # default: controller.go:377-383
            self.scale_delta[g] = int(r["delta"])                         # state.scaleDelta = delta, controller.go:434
            out.append(r)
        return out

    def scale_node_group(self, name: str, list_pods, list_nodes) -> tuple[int, str | None]:
        """(*Controller).scaleNodeGroup — controller.go:192, for one named group."""
        g = next(i for i, s in enumerate(self.groups) if s["name"] == name)
        r = self.run_once(list_pods, list_nodes)[g]
        return r["delta"], r["err"]


class _NodeNames:
    """names[j] for the walks, over the queue's index -> name map."""

    def __init__(self, events):
        self._events = events

    def __getitem__(self, j):
        return self._events.node_name(j)


class ResidentController(Controller):
    """RunOnce on the resident snapshot: no listers, no reload per scan.

    The caller feeds informer events to ``.events`` (escalator_amd/events.py: ``pod_add`` /
    ``pod_update`` / ``pod_delete``, ``node_add`` / ``node_update`` / ``node_delete``);
    ``run_once()`` flushes them into the device snapshot as batched patches (one reload when
    the ``spare`` room runs out), then decides, reaps and acts exactly as ``Controller`` does —
    the same host state, the same per-group result records, the same action switch.  Node
    indices handed to the actuator and returned in the records are snapshot indices
    (``events.node_name(j)`` names them).

    Wet mode: the actuator's taint / untaint / delete_nodes are API writes; the node Update or
    Delete they cause comes back as events the caller feeds to ``.events`` — the controller
    does not patch the snapshot behind the queue's back.  Dry mode: ``taint_tracker[g]`` stays
    the list of names (controller.go:35) and is mirrored onto the device with
    ``tracker_update`` after the walks; after a flush that added nodes or reloaded, tracked
    names the device does not track (a reload drops the tracker, a node back under a tracked
    name has a new index) are re-added; a tracked name whose node is gone stays in the list.

    ``audit_every=k`` (0 = never): on every k-th scan, after the flush and before the decision,
    ``ctx.audit()`` checks the snapshot's derived state against its primary tables; a mismatch
    reloads the snapshot once from the queue's object store (``events.reload_causes`` gets
    ``"audit:<check>"``) and counts in ``audit_failures``; ``audits`` counts the passes.

    ``pod_audit_every=k`` (keyword-only, 0 = never): the same schedule for ``ctx.audit_pods()``,
    the pod side's audit, after ``audit_every``'s pass when both fall on a scan; a mismatch reloads
    once (``"pod_audit:<check>"``); counters ``pod_audits``, ``pod_audit_failures``,
    ``last_pod_audit``.

    ``node_rebuild=True``: a ``nodes_add`` / ``nodes_relabel`` that runs out of node-side spare
    room is answered by ``ctx.nodes_rebuild()`` and one retry before any reload
    (``events.rebuild_causes``), and so is an audit mismatch confined to the state a rebuild
    re-derives (ENTRY, FIRST, REGION, OCC, TRACKER): those checks are run again after it, and
    only a mismatch that survives — or one in TOUCH or MIRROR — reloads.  The trackers outlive
    a rebuild, so nothing is re-added after one.

    ``node_compact=True`` (implies the rule above): a ``nodes_add`` that finds too few free
    table slots, and a ``pods_bind`` into a full run, are answered by ``ctx.nodes_compact()`` and
    one retry (``events.compact_causes``).  The node indices change with it; the tracker lists
    and instantiation times here are keyed by name, and the tracker pass that follows finds
    nothing missing.

    ``pod_grow=True``: a ``pods_upsert`` of more pods than the load left room for is answered by
    ``ctx.pods_grow()`` with the same batch and one retry before any reload
    (``events.pod_grows`` / ``events.pod_grow_causes``).  Pod ids, the placement, the trackers
    and the instantiation times stay; the next decision runs on a re-planned K1 grid.

    ``pod_compact=frac`` (off by default, ``None``): after a flush that applied cleanly the pod
    side is re-laid by ``ctx.pods_compact()`` when ``ctx.pods_slack()`` reports free tiles beyond
    the load's rule plus parked pods of at least ``frac`` of the live pods
    (``events.pod_compacts`` / ``events.pod_compact_causes``).  Pod ids and the placement stay.

    ``resync_every=k`` (keyword-only, off by default, ``None``): every k-th scan's flush is
    ``events.resync(ctx)`` — the flush, then every pod of the object store compared with the
    device (``ctx.pods_verify``) and what differs repaired through the event calls — before the
    audits and the decision; ``resyncs`` counts the passes, ``last_resync`` is the last result.

    ``node_resync_every=k`` (keyword-only, off by default, ``None``): every k-th scan runs
    ``events.resync_nodes(ctx)`` after the flush (or the pod resync) and before the audits and the
    decision — every node of the object store compared with the resident node table
    (``ctx.nodes_verify``) and what differs repaired through the node event calls;
    ``node_resyncs`` counts the passes, ``last_node_resync`` is the last result."""

    REBUILT_CHECKS = ("ENTRY", "FIRST", "REGION", "OCC", "TRACKER")
    # the pod audit is off unless the constructor's keyword turns it on
    pod_audit_every, pod_audits, pod_audit_failures, last_pod_audit = 0, 0, 0, None
    # and so is the resync of the pods' values
    resync_every, resyncs, last_resync = None, 0, None
    # and of the nodes'
    node_resync_every, node_resyncs, last_node_resync = None, 0, None

    def __init__(self, groups: list[dict], device: int = 0, dry_mode: bool = False, clock=None, actuator=None,
                 selection_slack: int = 4, spare: float = 0.5, audit_every: int = 0, node_rebuild: bool = False,
                 node_compact: bool = False, pod_grow: bool = False, *, pod_compact: float | None = None,
                 pod_audit_every: int = 0, resync_every: int | None = None,
                 node_resync_every: int | None = None):
        super().__init__(groups, device=device, dry_mode=dry_mode, clock=clock, actuator=actuator,
                         selection_slack=selection_slack)
        from .events import EventQueue
        self.spare = float(spare)
        self.node_compact = bool(node_compact)
        self.node_rebuild = bool(node_rebuild) or self.node_compact
        self.pod_grow = bool(pod_grow)
        self.events = EventQueue(spare=self.spare, rebuild=self.node_rebuild, compact=self.node_compact,
                                 pod_grow=self.pod_grow, pod_compact=pod_compact)
        # the resync of the derived state (the reference's informers resync hourly,
        # pkg/k8s/cache.go:27,48): every audit_every-th scan audits the snapshot after the flush
        # and reloads it once when a check finds a mismatch; 0 = never
        self.audit_every = int(audit_every)
        self.scans = 0
        self.audits = 0
        self.audit_failures = 0
        self.last_audit = None
        # the pod side's resync: every pod_audit_every-th scan runs ctx.audit_pods() after the
        # flush (and after audit_every's pass when both fall on a scan); 0 = never
        self.pod_audit_every = int(pod_audit_every)
        self.pod_audits = 0
        self.pod_audit_failures = 0
        self.last_pod_audit = None
        # the pods' values: every resync_every-th scan flushes through events.resync; None = never
        self.resync_every = int(resync_every) if resync_every else None
        self.resyncs = 0
        self.last_resync = None
        # the nodes' values: every node_resync_every-th scan runs events.resync_nodes; None = never
        self.node_resync_every = int(node_resync_every) if node_resync_every else None
        self.node_resyncs = 0
        self.last_node_resync = None

    def _learned(self, name: str, j: int, t: int):
        """The queue keeps the cache: it drops a name on node_delete and re-sends the cache
        after a reload (the only thing that loses the device's copy)."""
        self.events.inst_ns[name] = t

    def _sync_trackers(self):
        """filterNodes reads the tracker by name (controller.go:126-138): every tracked name
        with a live node is tracked on the device."""
        for g, names in self.taint_tracker.items():
            if not names:
                continue
            want = {self.events.node_index(n) for n in names} - {None}
            missing = sorted(want - set(int(j) for j in self.ctx.tracker_list(g)))
            if missing:
                self.ctx.tracker_update(g, add=missing)

    def _audit(self):
        """Context.audit on the flushed snapshot; a mismatch makes the queue reload once (cause
        "audit:<the first failing check>"), after which the trackers are re-added as after any
        reload."""
        self.last_audit = rep = self.ctx.audit()
        self.audits += 1
        bad = [n for n in L.AUDIT_CHECKS if n in rep and rep[n]["n_bad"] > 0]
        if bad:
            self.audit_failures += 1
            if getattr(self, "node_rebuild", False) and all(n in self.REBUILT_CHECKS for n in bad):
                self.events.node_rebuild(self.ctx, "audit:" + bad[0])
                again = self.ctx.audit(list(self.REBUILT_CHECKS))
                bad = [n for n in self.REBUILT_CHECKS if n in again and again[n]["n_bad"] > 0]
                if not bad:
                    return
            self.events.reload(self.ctx, "audit:" + bad[0])

    def _pod_audit(self):
        """Context.audit_pods on the flushed snapshot; a mismatch reloads once (cause
        "pod_audit:<the first failing check>"): nothing is repaired in place."""
        self.last_pod_audit = rep = self.ctx.audit_pods()
        self.pod_audits += 1
        bad = [n for n in L.POD_AUDIT_CHECKS if n in rep and rep[n]["n_bad"] > 0]
        if bad:
            self.pod_audit_failures += 1
            self.events.reload(self.ctx, "pod_audit:" + bad[0])

    def run_once(self) -> list[dict]:
        if self.resync_every and (self.scans + 1) % self.resync_every == 0:
            self.last_resync = self.events.resync(self.ctx)      # (flushes first)
            self.resyncs += 1
        else:
            self.events.flush(self.ctx)
        self.scans += 1
        if self.node_resync_every and self.scans % self.node_resync_every == 0:
            touched = self.events.touched_nodes                 # (its own flush resets the flag)
            self.last_node_resync = self.events.resync_nodes(self.ctx)
            self.events.touched_nodes = self.events.touched_nodes or touched
            self.node_resyncs += 1
        if self.audit_every and self.scans % self.audit_every == 0:
            self._audit()
        if self.pod_audit_every and self.scans % self.pod_audit_every == 0:
            self._pod_audit()
        if self.events.touched_nodes:
            self._sync_trackers()
        now = self.clock()
        self._lock_states(now)
        tot, dec = self.ctx.decide_all(self.state)       # the ordering is in the step
        try:
            self._sel = self.ctx.selections()
        except L.EscError as e:
            if e.code != L.ESC_E_ORDER:
                raise
            self._sel = None
            self.ctx.sort_nodes()
        soft = [int(grp.get("soft_delete_grace_ns", 0)) for grp in self.groups]
        hard = [int(grp.get("hard_delete_grace_ns", 0)) for grp in self.groups]
        self._removal = self.ctx.try_remove(now, soft, hard)
        names = _NodeNames(self.events)
        self._new_nodes = self._new_node_pass(dec, names)
        out = self._act(tot, dec, names)
        for g, r in enumerate(out):                      # the dry-mode walks' tracker changes
            if self.groups[g]["dry_mode"] and (r.get("tainted_now") or r.get("untainted_now")):
                self.ctx.tracker_update(g, add=r.get("tainted_now", []), remove=r.get("untainted_now", []))
        return out
