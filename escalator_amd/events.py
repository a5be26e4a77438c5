"""The informer cache in front of the resident snapshot: identities -> snapshot indices.

``EventQueue`` plays the reference's informer cache feeding the listers
(pkg/k8s/cache.go:16-56, pod_listers.go:33-49, node_listers.go:33-48) plus the identity
maps the event calls of the C ABI need: every ``esc_pods_*`` / ``esc_nodes_*`` call takes
snapshot indices, and this queue is what maps a pod key or a node name to one, hands out and
recycles pod ids, batches a scan's events into at most one call per kind and falls back to
one full reload when ``ESC_E_LIMIT`` says the spare room ran out.  With ``rebuild=True`` a
node call that answers ``ESC_E_LIMIT`` is first answered by ``nodes_rebuild`` (the node side
re-derived on the device, no pod reloaded) and retried once.  With ``compact=True`` a
``nodes_add`` that lacks free table slots, and a ``pods_bind`` into a full run, are answered by
``nodes_compact`` (the live nodes renumbered into a fresh table on the device, the runs re-cut)
and retried once; the queue's index maps follow the returned map.  With ``pod_grow=True`` a
``pods_upsert`` that answers ``ESC_E_LIMIT`` (more pods than the load left room for) is answered
by one ``pods_grow`` with the same ids and packed batch (the pod classes grown on the device, no
pod reloaded, every id kept) and one retry; a second limit reloads.  With ``pod_compact=frac`` a
flush that applied cleanly is followed by one ``pods_compact`` (the pod side re-laid on the device:
classes shrunk to the load's rule, parked pods back in their classes, every id kept) when
``pods_slack`` reports ``(k_tiles - k_tiles_rule) * 256 + parked >= frac * live pods``.
``resync(ctx)`` is the informers' periodic resync: the whole object store compared with the device
(``pods_verify``) and only what differs repaired through the calls above; ``resync_nodes(ctx)`` is
the same for the nodes (``nodes_verify``: labels, creation time, cordon, taint, allocatable, taint
time, no-delete flag, instantiation time).

It holds the current objects (plain-dict records, escalator_amd/objects.py) — the truth a
reload is built from — and, beside them, what the device last saw of each.  Ingest
(``pod_add`` ... ``node_delete``) only changes the object store and marks the key dirty;
``flush(ctx)`` diffs the dirty keys against the device's view, so events on one key coalesce
(the last write wins, an add and a delete of a key the device never saw cancel) without a
log.  Records are values: an update hands in a new dict, it does not change the one the
queue holds.  ``ctx`` is anything with ``Context``'s methods.
"""
from __future__ import annotations

import heapq
import logging

import numpy as np

from ._lib import ESC_E_LIMIT, ESC_E_STATE
from .objects import NO_DELETE_ANNOTATION, TO_BE_REMOVED_KEY, placement, taint_time

NONE = 0xFFFFFFFF
KINDS = ("nodes_delete", "nodes_add", "nodes_relabel", "nodes_update", "nodes_facts",
         "pods_delete", "pods_upsert", "pods_bind")
# the pod fields the packed record is built from (objects.pods_to_c)
_POD_SPEC = ("owner_kinds", "node_selector", "affinity", "containers", "init_containers", "overhead")


class _Reload(Exception):
    """A batched call answered ESC_E_LIMIT: the rest of the batch is abandoned."""


def pod_key(pod: dict) -> str:
    ns = pod.get("namespace")
    return "%s/%s" % (ns, pod.get("name", "")) if ns else pod.get("name", "")


def _pod_spec(p: dict):
    src = (p.get("annotations") or {}).get("kubernetes.io/config.source")
    return [p.get(k) or None for k in _POD_SPEC] + [src]


def _no_delete(n: dict) -> int:
    return 1 if (n.get("annotations") or {}).get(NO_DELETE_ANNOTATION, "") else 0


def _facts(n: dict):
    return taint_time(n), _no_delete(n)


def _shape(n: dict):
    """What esc_nodes_relabel carries beyond esc_nodes_update."""
    return n.get("labels") or {}, int(n.get("created_ns", 0))


def _status(n: dict):
    """What esc_nodes_update may change: cordon, escalator-taint presence, allocatable."""
    return (bool(n.get("unschedulable")), TO_BE_REMOVED_KEY in (n.get("taints") or []),
            n.get("cpu") or 0, n.get("mem") or 0)


class EventQueue:
    def __init__(self, spare: float = 0.5, rebuild: bool = False, compact: bool = False, pod_grow: bool = False,
                 pod_compact: float | None = None):
        self.spare = float(spare)
        self.compact = bool(compact)               # answer a lack of table slots / a full run with nodes_compact
        self.rebuild = bool(rebuild) or self.compact   # answer a node-side ESC_E_LIMIT with nodes_rebuild first
        self.rebuilds = 0
        self.rebuild_causes: list[str] = []        # the call that answered ESC_E_LIMIT, or "audit:<check>"
        self.compactions = 0
        self.compact_causes: list[str] = []        # the call that answered ESC_E_LIMIT
        self.pod_grow = bool(pod_grow)             # answer a full pod class / C section with pods_grow
        self.pod_grows = 0
        self.pod_grow_causes: list[str] = []       # the call that answered ESC_E_LIMIT
        # re-lay the pod side (pods_compact) once its slack reaches this fraction of the live pods
        self.pod_compact = None if pod_compact is None else float(pod_compact)
        self.pod_compacts = 0
        self.pod_compact_causes: list[str] = []    # "slack" (free tiles alone reach the threshold) / "parked"
        self.pod_compact_failures = 0
        self.resyncs = 0                           # resync() calls, and the pods each kind of repair took
        self.resync_repairs = {"absent": 0, "class": 0, "value": 0, "bind": 0, "orphans": 0}
        self.node_resyncs = 0                      # resync_nodes() calls, and the nodes each kind of repair took
        self.node_resync_repairs = {"absent": 0, "shape": 0, "status": 0, "facts": 0, "inst": 0, "orphans": 0}
        self.pods: dict[str, dict] = {}            # the object store: key -> pod, name -> node
        self.nodes: dict[str, dict] = {}           # (insertion order = arrival order)
        self._dev_pods: dict[str, dict] = {}       # the records the device holds, as last flushed
        self._dev_nodes: dict[str, dict] = {}
        self._node_idx: dict[str, int] = {}
        self._idx_node: dict[int, str] = {}
        self._pod_id: dict[str, int] = {}
        self._free: list[int] = []                 # heap of freed pod ids
        self._next_id = 0
        self._by_node: dict[str, set] = {}         # node name -> keys of pods whose node_name is it
        self._dirty_pods: dict[str, bool] = {}     # key -> deleted since the last flush (re-add = fresh)
        self._dirty_nodes: dict[str, bool] = {}
        self._loaded = False
        self.reloads = 0
        self.reload_causes: list[str] = []         # "first", the call that answered ESC_E_LIMIT, or "audit:<check>"
        self.flushes = 0
        self.applied = {k: 0 for k in KINDS}
        self.touched_nodes = False                 # the last flush added nodes or reloaded
        # node name -> the cloud instance's instantiation time (Unix ns), as the controller's
        # new-node pass learned it (GetInstance, controller.go:173): the device holds the
        # same fact per slot, and only a reload loses it there
        self.inst_ns: dict[str, int] = {}

    # ------------------------------------------------------------------ ingest
    def _index_pod(self, key, old, new):
        for p, add in ((old, False), (new, True)):
            name = (p or {}).get("node_name") or ""
            if not name:
                continue
            s = self._by_node.setdefault(name, set())
            (s.add if add else s.discard)(key)
            if not s:
                del self._by_node[name]

    def pod_add(self, pod: dict):
        key = pod_key(pod)
        self._index_pod(key, self.pods.get(key), pod)
        self.pods[key] = pod
        self._dirty_pods.setdefault(key, False)

    pod_update = pod_add

    def pod_delete(self, pod):
        key = pod if isinstance(pod, str) else pod_key(pod)
        old = self.pods.pop(key, None)
        if old is None:
            return
        self._index_pod(key, old, None)
        self._dirty_pods[key] = True

    def node_add(self, node: dict):
        name = node.get("name", "")
        self.nodes[name] = node                    # back after a delete: listed last again
        self._dirty_nodes.setdefault(name, False)

    node_update = node_add

    def node_delete(self, node):
        name = node if isinstance(node, str) else node.get("name", "")
        self.inst_ns.pop(name, None)               # a node back under this name is a new instance
        if self.nodes.pop(name, None) is not None:
            self._dirty_nodes[name] = True

    # ------------------------------------------------------------------ lookups
    def node_index(self, name: str):
        return self._node_idx.get(name)

    def node_name(self, index: int):
        return self._idx_node.get(int(index))

    def pod_id(self, key: str):
        return self._pod_id.get(key)

    def live_nodes(self) -> list[dict]:
        """The device's nodes in snapshot-index order (the lister order)."""
        return [self._dev_nodes[self._idx_node[j]] for j in sorted(self._idx_node)]

    def live_pods(self) -> list[dict]:
        return [self._dev_pods[k] for k in sorted(self._pod_id, key=self._pod_id.get)]

    # ------------------------------------------------------------------ flush
    def _take_id(self) -> int:
        if self._free:
            return heapq.heappop(self._free)
        self._next_id += 1
        return self._next_id - 1

    def _call(self, kind: str, n: int, fn, *args):
        try:
            rc = fn(*args)
        except Exception as e:
            if getattr(e, "code", None) == ESC_E_LIMIT:
                raise _Reload(kind) from None
            raise
        if kind == "pods_upsert" and rc == ESC_E_LIMIT:    # the one call that returns its code
            raise _Reload(kind)
        self.applied[kind] += n
        return rc

    def _node_call(self, ctx, kind: str, n: int, slots: int, xl_words: int, fn, *args):
        """A nodes_add / nodes_relabel call: with ``rebuild`` on, its first ESC_E_LIMIT is
        answered by one node-side rebuild (when the table has the `slots` free slots the call
        needs: a rebuild does not grow the table) and one retry; the second reloads.  With
        ``compact`` on, too few free slots are answered by one compaction (which includes the
        rebuild) with room for the batch's `slots` and `xl_words`, and one retry."""
        try:
            return self._call(kind, n, fn, *args)
        except _Reload:
            if not self.rebuild:
                raise
            short = bool(slots) and ctx.nodes_room()[0] < slots
            if short and not self.compact:
                raise
        if short:
            self.node_compact(ctx, kind, slots, xl_words)
        else:
            self.node_rebuild(ctx, kind)
        return self._call(kind, n, fn, *args)

    def node_rebuild(self, ctx, cause: str):
        """One ``nodes_rebuild``: `cause` goes into ``rebuild_causes``.  Indices, pods, the
        placement, the trackers and the instantiation times stay as they are."""
        ctx.nodes_rebuild()
        self.rebuilds += 1
        self.rebuild_causes.append(cause)

    def node_compact(self, ctx, cause: str, slots: int = 0, xl_words: int = 0):
        """One ``nodes_compact``: `cause` goes into ``compact_causes`` and the index maps follow
        the returned map (in place: a flush in progress holds them).  Pods, the trackers and
        the instantiation times stay as they are."""
        new = ctx.nodes_compact(min_free_slots=slots, min_free_xl_words=xl_words)
        moved = {m: int(new[j]) for m, j in self._node_idx.items()}
        assert all(j >= 0 for j in moved.values()), "a node the queue holds was absent on the device"
        self._node_idx.clear()
        self._node_idx.update(moved)
        self._idx_node.clear()
        self._idx_node.update((j, m) for m, j in moved.items())
        self.compactions += 1
        self.compact_causes.append(cause)
        self.touched_nodes = True

    def _target(self, pod: dict) -> int:
        return self._node_idx.get(pod.get("node_name") or "", NONE) if pod.get("node_name") else NONE

    def flush(self, ctx):
        """Applies what was ingested since the last flush: at most one call per kind, node
        calls first (pods bind to nodes), or one reload."""
        self.flushes += 1
        self.touched_nodes = False
        dirty_p, dirty_n = self._dirty_pods, self._dirty_nodes
        self._dirty_pods, self._dirty_nodes = {}, {}
        if not self._loaded:
            ctx.set_spare(self.spare)
            self.reload_causes.append("first")
            return self._reload(ctx, dirty_p, dirty_n)
        try:
            self._apply(ctx, dirty_p, dirty_n)
        except _Reload as e:
            self.reload_causes.append(str(e))
            return self._reload(ctx, dirty_p, dirty_n)
        if self.pod_compact is not None:
            self._maybe_compact_pods(ctx)

    def _maybe_compact_pods(self, ctx):
        """After a flush that applied cleanly: one ``pods_compact`` when the free tiles beyond
        the load's rule and the parked pods together reach ``pod_compact`` of the live pods.  A
        compaction that fails before its swap changed nothing: logged, counted and ignored.
        One that fails after it leaves the context stale (``pods_slack`` then answers
        ESC_E_STATE): the snapshot is reloaded at once, cause ``"pods_compact"``."""
        s = ctx.pods_slack()
        tiles = (s["k_tiles"] - s["k_tiles_rule"]) * 256
        need = self.pod_compact * len(self._pod_id)
        if tiles + s["parked"] <= 0 or tiles + s["parked"] < need:
            return
        try:
            ctx.pods_compact()
        except Exception as e:
            if getattr(e, "code", None) is None:
                raise
            self.pod_compact_failures += 1
            log = logging.getLogger(__name__)
            try:
                ctx.pods_slack()
            except Exception as e2:
                if getattr(e2, "code", None) != ESC_E_STATE:
                    raise
                log.warning("pods_compact failed after its swap (%s): the snapshot is stale and is reloaded", e)
                self.reload_causes.append("pods_compact")
                self._reload(ctx, {}, {})
                return
            log.warning("pods_compact failed before its swap (%s): the snapshot stays as it is", e)
            return
        self.pod_compacts += 1
        self.pod_compact_causes.append("slack" if tiles > 0 and tiles >= need else "parked")

    def reload(self, ctx, cause: str):
        """One full load from the object store outside a flush (a failed audit): `cause` goes
        into ``reload_causes``, whatever was ingested since the last flush is taken along."""
        if not self._loaded:
            return self.flush(ctx)
        dirty_p, dirty_n = self._dirty_pods, self._dirty_nodes
        self._dirty_pods, self._dirty_nodes = {}, {}
        self.reload_causes.append(cause)
        self._reload(ctx, dirty_p, dirty_n)

    def _apply(self, ctx, dirty_p, dirty_n):
        dev_n, idx = self._dev_nodes, self._node_idx
        # --- nodes: delete, add, then the three kinds of update
        gone = [m for m, fresh in dirty_n.items() if m in dev_n and (fresh or m not in self.nodes)]
        if gone:
            self._call("nodes_delete", len(gone), ctx.nodes_delete, np.array([idx[m] for m in gone], np.int64))
            for m in gone:
                del self._idx_node[idx.pop(m)]
                del dev_n[m]
        new = [m for m in self.nodes if m in dirty_n and m not in dev_n]
        if new:
            _, packed = ctx.pack([], [self.nodes[m] for m in new])
            ids = self._node_call(ctx, "nodes_add", len(new), len(new), len(packed.get("xl_pair", ())), ctx.nodes_add,
                                  packed)
            for m, j in zip(new, ids):
                idx[m] = int(j)
                self._idx_node[int(j)] = m
                dev_n[m] = self.nodes[m]
            self.touched_nodes = True
        fresh_nodes = set(new)
        relabel, update, facts = [], [], list(new)
        for m in dirty_n:
            if m in fresh_nodes or m not in self.nodes:
                continue
            old, cur = dev_n[m], self.nodes[m]
            if _shape(old) != _shape(cur):
                relabel.append(m)
            elif _status(old) != _status(cur):
                update.append(m)
            if _facts(old) != _facts(cur):
                facts.append(m)
        if relabel:
            _, packed = ctx.pack([], [self.nodes[m] for m in relabel])
            self._node_call(ctx, "nodes_relabel", len(relabel), 0, 0, ctx.nodes_relabel,
                            np.array([idx[m] for m in relabel], np.int64), packed)
        if update:
            _, packed = ctx.pack([], [self.nodes[m] for m in update])
            self._call("nodes_update", len(update), ctx.nodes_update, np.array([idx[m] for m in update], np.int64),
                       packed["flags"], packed["cpu"], packed["mem"])
        if facts:
            f = [_facts(self.nodes[m]) for m in facts]
            self._call("nodes_facts", len(facts), ctx.nodes_facts, np.array([idx[m] for m in facts], np.int64),
                       np.array([t for t, _ in f], np.int64), np.array([d for _, d in f], np.uint8))
        for m in dirty_n:
            if m in self.nodes:
                dev_n[m] = self.nodes[m]
        # --- pods: delete, upsert, bind
        dev_p, pid = self._dev_pods, self._pod_id
        gone = [k for k, fresh in dirty_p.items() if k in dev_p and (fresh or k not in self.pods)]
        if gone:
            self._call("pods_delete", len(gone), ctx.pods_delete, np.array([pid[k] for k in gone], np.int64))
            for k in gone:
                heapq.heappush(self._free, pid.pop(k))
                del dev_p[k]
        born = [k for k in self.pods if k in dirty_p and k not in dev_p]
        changed = [k for k in dirty_p if k in dev_p and k in self.pods]
        upsert = born + [k for k in changed if _pod_spec(dev_p[k]) != _pod_spec(self.pods[k])]
        for k in born:
            pid[k] = self._take_id()
        self._upsert_pods(ctx, upsert)
        bind = list(born)
        seen = set(born)
        for k in changed:
            if (dev_p[k].get("node_name") or "") != (self.pods[k].get("node_name") or ""):
                bind.append(k)
                seen.add(k)
        for m in new:                                      # pods that named the node before it came
            for k in sorted(self._by_node.get(m, ()), key=lambda k: pid.get(k, -1)):
                if k not in seen and k in pid:
                    bind.append(k)
                    seen.add(k)
        for k in dirty_p:
            if k in self.pods:
                dev_p[k] = self.pods[k]
        self._bind_pods(ctx, bind)

    def _upsert_pods(self, ctx, keys):
        """One ``pods_upsert`` of the store's pods `keys` under their ids; with ``pod_grow`` on
        its first ESC_E_LIMIT is answered by one ``pods_grow`` and one retry."""
        if not keys:
            return
        pid = self._pod_id
        packed, _ = ctx.pack([self.pods[k] for k in keys], [])
        ids = np.array([pid[k] for k in keys], np.int64)
        try:
            self._call("pods_upsert", len(keys), ctx.pods_upsert, ids, packed)
        except _Reload:
            if not self.pod_grow:
                raise
            # a full class or C section: grown on the device for this batch, then one retry
            self._call("pods_upsert", 0, ctx.pods_grow, ids, packed)
            self.pod_grows += 1
            self.pod_grow_causes.append("pods_upsert")
            self._call("pods_upsert", len(keys), ctx.pods_upsert, ids, packed)

    def _bind_pods(self, ctx, keys):
        """One ``pods_bind`` of the store's pods `keys` to their nodes; with ``compact`` on a full
        run is answered by one ``nodes_compact`` and one retry."""
        if not keys:
            return
        ids = np.array([self._pod_id[k] for k in keys], np.int64)
        try:
            self._call("pods_bind", len(keys), ctx.pods_bind, ids,
                       np.array([self._target(self.pods[k]) for k in keys], np.uint32))
        except _Reload:
            if not self.compact:
                raise
            # a full run: the compaction re-cuts the runs (the targets' indices change with it)
            self.node_compact(ctx, "pods_bind")
            self._call("pods_bind", len(keys), ctx.pods_bind, ids,
                       np.array([self._target(self.pods[k]) for k in keys], np.uint32))

    # ------------------------------------------------------------------ resync
    def resync(self, ctx, chunk: int = 65536) -> dict:
        """The informers' resync (pkg/k8s/cache.go:27,48) for the resident snapshot: after a
        flush, every pod of the object store is packed as a flush packs it and compared with what
        its slot holds on the device (``pods_verify``, `chunk` pods per call), bindings included,
        and the device's live ids are compared with the identity map.  What differs is repaired
        through the flush's own paths, an ESC_E_LIMIT answered as a flush answers it
        (``pods_grow`` / ``nodes_compact`` when enabled, else one reload): the pods reported
        absent, of another class or with another value in one ``pods_upsert``, the pods bound
        elsewhere in one ``pods_bind``, the ids no pod of the store has in one ``pods_delete``.
        Returns ``{checked, absent, class, value, bind, orphans, reloaded}``."""
        from ._lib import PV_ABSENT, PV_BIND, PV_CLASS, PV_VALUE
        self.flush(ctx)
        self.resyncs += 1
        pid = self._pod_id
        out = {"checked": 0, "absent": 0, "class": 0, "value": 0, "bind": 0, "orphans": 0, "reloaded": False}
        keys = [k for k in self.pods if k in pid]
        upsert, bind = [], []
        for a in range(0, len(keys), max(1, int(chunk))):
            ks = keys[a:a + max(1, int(chunk))]
            packed, _ = ctx.pack([self.pods[k] for k in ks], [])
            status, _rep = ctx.pods_verify(np.array([pid[k] for k in ks], np.int64), packed,
                                           np.array([self._target(self.pods[k]) for k in ks], np.uint32))
            status = np.asarray(status, np.uint8)
            out["checked"] += len(ks)
            for name, bit in (("absent", PV_ABSENT), ("class", PV_CLASS), ("value", PV_VALUE), ("bind", PV_BIND)):
                out[name] += int(np.count_nonzero(status & bit))
            upsert += [ks[i] for i in np.flatnonzero(status & (PV_ABSENT | PV_CLASS | PV_VALUE))]
            bind += [ks[i] for i in np.flatnonzero(status & PV_BIND)]
        # the other direction: ids the device holds for no pod of the store (an id the map still
        # names for a key the store lost is one of them: its delete never arrived)
        known = {pid[k] for k in keys}
        orphans = [int(i) for i in ctx.pods_live_ids() if int(i) not in known]
        out["orphans"] = len(orphans)
        log = logging.getLogger(__name__)
        for name in ("absent", "class", "value", "bind", "orphans"):
            if out[name]:
                self.resync_repairs[name] += out[name]
                log.warning("resync: %d pods %s", out[name],
                            {"absent": "missing on the device", "class": "in another class on the device",
                             "value": "with other values on the device", "bind": "bound elsewhere on the device",
                             "orphans": "on the device and not in the store"}[name])
        try:
            self._upsert_pods(ctx, upsert)
            self._bind_pods(ctx, bind)
            if orphans:
                self._call("pods_delete", len(orphans), ctx.pods_delete, np.array(orphans, np.int64))
        except _Reload as e:
            self.reload_causes.append("resync:%s" % e)
            self._reload(ctx, {}, {})
            out["reloaded"] = True
            return out
        for k in upsert + bind:
            self._dev_pods[k] = self.pods[k]
        gone = set(orphans)
        for k in [k for k, i in pid.items() if i in gone and k not in self.pods]:
            heapq.heappush(self._free, pid.pop(k))
            self._dev_pods.pop(k, None)
        return out

    def resync_nodes(self, ctx, chunk: int = 65536) -> dict:
        """The node half of the informers' resync: after a flush, every node of the object store
        that has an index is packed as a flush packs it and compared with the resident node table
        (``nodes_verify``, `chunk` nodes per call) together with its facts (taint time, no-delete)
        and the instantiation time the queue holds for it (unknown otherwise); the device's live
        slots are compared with the identity map.  What differs is repaired through the flush's
        own calls in the flush's order, an ESC_E_LIMIT answered as a flush answers it
        (``nodes_rebuild`` / ``nodes_compact`` when enabled, else one reload): the slots no node of
        the map has in one ``nodes_delete``; the nodes reported absent lose their index and are
        added again (``nodes_add``, their pods bound again); the nodes of another shape in one
        ``nodes_relabel`` (which rewrites the status too); the others of another status in one
        ``nodes_update``; other facts in one ``nodes_facts``; other instantiation times in one
        ``nodes_instantiated``.  Returns ``{checked, absent, shape, status, facts, inst, orphans,
        reloaded}``."""
        from ._lib import NV_ABSENT, NV_FACTS, NV_INST, NV_SHAPE, NV_STATUS
        self.flush(ctx)
        self.node_resyncs += 1
        idx = self._node_idx
        unknown = -(1 << 63)
        bits = (("absent", NV_ABSENT), ("shape", NV_SHAPE), ("status", NV_STATUS), ("facts", NV_FACTS), ("inst", NV_INST))
        out = {"checked": 0, "absent": 0, "shape": 0, "status": 0, "facts": 0, "inst": 0, "orphans": 0, "reloaded": False}
        names = [m for m in self.nodes if m in idx]
        found = {name: [] for name, _ in bits}
        for a in range(0, len(names), max(1, int(chunk))):
            ms = names[a:a + max(1, int(chunk))]
            _, packed = ctx.pack([], [self.nodes[m] for m in ms])
            f = [_facts(self.nodes[m]) for m in ms]
            status, _rep = ctx.nodes_verify(np.array([idx[m] for m in ms], np.int64), packed,
                                            np.array([t for t, _ in f], np.int64), np.array([d for _, d in f], np.uint8),
                                            np.array([self.inst_ns.get(m, unknown) for m in ms], np.int64))
            status = np.asarray(status, np.uint8)
            out["checked"] += len(ms)
            for name, bit in bits:
                found[name] += [ms[i] for i in np.flatnonzero(status & bit)]
        # the other direction: live slots the identity map does not name (their delete never arrived)
        orphans = [int(j) for j in ctx.nodes_live_ids() if int(j) not in self._idx_node]
        out["orphans"] = len(orphans)
        log = logging.getLogger(__name__)
        for name in ("absent", "shape", "status", "facts", "inst", "orphans"):
            if name != "orphans":
                out[name] = len(found[name])
            if out[name]:
                self.node_resync_repairs[name] += out[name]
                log.warning("resync: %d nodes %s", out[name],
                            {"absent": "missing on the device", "shape": "with other labels or creation time on the device",
                             "status": "with another cordon, taint or allocatable on the device",
                             "facts": "with another taint time or no-delete flag on the device",
                             "inst": "with another instantiation time on the device",
                             "orphans": "on the device and not in the store"}[name])
        absent = found["absent"]
        shaped = set(found["shape"])
        relabel = found["shape"]
        update = [m for m in found["status"] if m not in shaped]
        facts = absent + found["facts"]
        inst = [m for m in absent if m in self.inst_ns] + found["inst"]
        try:
            if orphans:
                self._call("nodes_delete", len(orphans), ctx.nodes_delete, np.array(orphans, np.int64))
            if absent:
                for m in absent:                               # the index names no node: the node is new again
                    self._idx_node.pop(idx.pop(m), None)
                    self._dev_nodes.pop(m, None)
                _, packed = ctx.pack([], [self.nodes[m] for m in absent])
                ids = self._node_call(ctx, "nodes_add", len(absent), len(absent), len(packed.get("xl_pair", ())),
                                      ctx.nodes_add, packed)
                for m, j in zip(absent, ids):
                    idx[m] = int(j)
                    self._idx_node[int(j)] = m
                self.touched_nodes = True
            if relabel:
                _, packed = ctx.pack([], [self.nodes[m] for m in relabel])
                self._node_call(ctx, "nodes_relabel", len(relabel), 0, 0, ctx.nodes_relabel,
                                np.array([idx[m] for m in relabel], np.int64), packed)
            if update:
                _, packed = ctx.pack([], [self.nodes[m] for m in update])
                self._call("nodes_update", len(update), ctx.nodes_update, np.array([idx[m] for m in update], np.int64),
                           packed["flags"], packed["cpu"], packed["mem"])
            if facts:
                f = [_facts(self.nodes[m]) for m in facts]
                self._call("nodes_facts", len(facts), ctx.nodes_facts, np.array([idx[m] for m in facts], np.int64),
                           np.array([t for t, _ in f], np.int64), np.array([d for _, d in f], np.uint8))
            if inst:
                ctx.nodes_instantiated(np.array([idx[m] for m in inst], np.int64),
                                       np.array([self.inst_ns.get(m, unknown) for m in inst], np.int64))
            # the pods that name a node added again, as for a node that arrives after its pods
            pid = self._pod_id
            bind = [k for m in absent for k in sorted(self._by_node.get(m, ()), key=lambda k: pid.get(k, -1)) if k in pid]
            self._bind_pods(ctx, bind)
        except _Reload as e:
            self.reload_causes.append("resync_nodes:%s" % e)
            self._reload(ctx, {}, {})
            out["reloaded"] = True
            return out
        for m in absent + relabel + update + facts:
            self._dev_nodes[m] = self.nodes[m]
        return out

    def _reload(self, ctx, dirty_p, dirty_n):
        """One full load from the object store: the nodes the device held keep their order
        (compacted in snapshot-index order, so allNodes[0] and the tie order stay), nodes it
        never held follow in arrival order — a node deleted and added again under its name
        since the device saw it among them; pods are renumbered the same way."""
        order_n = [m for m in sorted(self._node_idx, key=self._node_idx.get)
                   if m in self.nodes and not dirty_n.get(m)]
        keep = set(order_n)
        order_n += [m for m in self.nodes if m not in keep]
        had = [k for k in sorted(self._pod_id, key=self._pod_id.get) if k in self.pods and not dirty_p.get(k)]
        keep = set(had)
        order_p = had + [k for k in self.pods if k not in keep]
        nodes = [self.nodes[m] for m in order_n]
        pods = [self.pods[k] for k in order_p]
        P, N = ctx.pack(pods, nodes)
        ctx.load(P, N)
        ctx.load_placement(*placement(pods, nodes))
        self._node_idx = {m: j for j, m in enumerate(order_n)}
        self._idx_node = dict(enumerate(order_n))
        self._pod_id = {k: i for i, k in enumerate(order_p)}
        self._free, self._next_id = [], len(order_p)
        self._dev_nodes = dict(zip(order_n, nodes))
        self._dev_pods = dict(zip(order_p, pods))
        self._loaded = True
        self.touched_nodes = True
        self.reloads += 1
        # the load left every instantiation time unknown: the known ones go back in one call
        known = [m for m in order_n if m in self.inst_ns]
        if known:
            ctx.nodes_instantiated(np.array([self._node_idx[m] for m in known], np.int64),
                                   np.array([self.inst_ns[m] for m in known], np.int64))
