"""The cluster of tests/test_gpu_inert.py and its child process (tests/inert_child.py): five groups,
each under a pair of its own key ("k0" .. "k4", value "v"), optionally a sixth named "default", and
pods at every edge of the definition of an inert pod times 0 .. 3 extra pairs.

A pod's pairs are the entries of its selector whose key some group uses; (k_i, "v") is group i's
pair (ids 0 .. 4 in group order, so group 4's is n_gp - 1) and (k_i, "x") a pair no group selects
(ids from n_gp on).  The pairs sort by id, so a pod's group pairs come first.  A pod with p pairs
has p - 1 extra pairs; ``N_INERT[x]`` / ``N_LIVE[x]`` pods sit in the inert class and in the packed
small class of x extra pairs: 255, 256 and 257, one tile's edge each way."""
N_GROUPS = 5
N_INERT = {0: 256, 1: 255, 2: 257, 3: 256}
N_LIVE = {0: 257, 1: 256, 2: 255, 3: 257}
TAINT = "atlassian.com/escalator"
T0 = 1_700_000_000 * 10**9
NOW = T0 + 10**12


def groups(with_default):
    out = [{"name": "g%d" % i, "label_key": "k%d" % i, "label_value": "v", "min_nodes": 0, "max_nodes": 5000,
            "taint_lower_pct": 20, "taint_upper_pct": 40, "scale_up_pct": 70, "slow_removal_rate": 1,
            "fast_removal_rate": 2, "dry_mode": False} for i in range(N_GROUPS)]
    if with_default:
        out.append(dict(out[0], name="default", label_key="", label_value=""))
    return out


def pod(name, sel=None, ds=False, static=False, aff=False, cpu=100, mem=1 << 20, node_name=""):
    return {"name": name, "owner_kinds": ["ReplicaSet", "DaemonSet"] if ds else [],
            "annotations": {"kubernetes.io/config.source": "file"} if static else {},
            "node_selector": sel, "node_name": node_name,
            "affinity": {"node_affinity": None, "pod_affinity": True, "pod_anti_affinity": False} if aff else None,
            "containers": [{"cpu": cpu, "mem": mem}], "init_containers": [], "overhead": None}


def live_sel(g, x):
    """Group g's pair and x pairs no group selects."""
    sel = {"k%d" % g: "v"}
    for j in range(1, x + 1):
        sel["k%d" % ((g + j) % N_GROUPS)] = "x"
    return sel


def other_sel(x, first=0):
    """x + 1 pairs no group selects."""
    return {"k%d" % ((first + j) % N_GROUPS): "x" for j in range(x + 1)}


def inert_kinds(x):
    """(kind, pod keywords) of the inert pods with x extra pairs."""
    k = [("ds_group_pair", dict(sel=live_sel(2, x), ds=True)),
         ("sel_other_pairs", dict(sel=other_sel(x))),
         ("static_other_pairs", dict(sel=other_sel(x, 3), static=True)),
         ("aff_other_pairs", dict(sel=other_sel(x, 1), aff=True))]
    if x == 0:
        k += [("ds_no_pair", dict(ds=True)), ("static", dict(static=True)), ("aff_only", dict(aff=True)),
              ("sel_foreign_key", dict(sel={"zone": "a"})), ("sel_first_other_pair", dict(sel={"k4": "x"}))]
    return k


def live_kinds(x):
    """(kind, pod keywords) of the counted pods with x extra pairs."""
    k = [("sel_group_pair", dict(sel=live_sel(0, x))), ("sel_last_group_pair", dict(sel=live_sel(4, x))),
         ("static_group_pair", dict(sel=live_sel(1, x), static=True)),
         ("aff_group_pair", dict(sel=live_sel(3, x), aff=True))]
    if x == 0:
        k += [("no_filter_bit", dict())]                   # joins the default filter's slot
    return k


def nodes():
    """Four nodes per group (one of them tainted long ago) and "lonely", a tainted node of group 0
    that only inert pods are bound to."""
    out = []
    for i in range(4 * N_GROUPS):
        nd = {"name": "n%d" % i, "labels": {"k%d" % (i % N_GROUPS): "v"}, "unschedulable": False, "taints": [],
              "cpu": 4000 + i % 7, "mem": (8 << 30) + i, "created_ns": T0 + i * 1000}
        if i >= 3 * N_GROUPS:
            nd.update(taints=[TAINT], taint_value=str(NOW // 10**9 - 900))
        out.append(nd)
    out.append(dict(out[-1], name="lonely", labels={"k0": "v"}, created_ns=T0 + 99_000))
    return out


def pods():
    """Returns (pods, kind of every pod, whether it is inert): the small pods of every kind, the
    classes filled to N_INERT / N_LIVE, then inert pods outside the packed small block."""
    out, kinds, inert = [], [], []

    def add(kind, is_inert, **kw):
        i = len(out)
        # every third pod bound: live ones to their group's nodes, inert ones to "lonely" too
        node_name = ("lonely" if is_inert and i % 2 else "n%d" % (i % 20)) if i % 3 == 0 else ""
        out.append(pod("p%d" % i, node_name=node_name, cpu=100 + i % 50, **kw))
        kinds.append(kind)
        inert.append(is_inert)

    for x in range(4):
        ik, lk = inert_kinds(x), live_kinds(x)
        for j in range(N_INERT[x]):
            add(*ik[j % len(ik)][:1], True, **ik[j % len(ik)][1])
        for j in range(N_LIVE[x]):
            add(*lk[j % len(lk)][:1], False, **lk[j % len(lk)][1])
    for j in range(5):                                     # inert, 12 B: the packed class, as before
        add("ds_12_bytes", True, ds=True, mem=1 << 34)
        add("static_12_bytes", True, static=True, sel=other_sel(j % 4), mem=1 << 34)
    add("ds_plain", True, ds=True, mem=1 << 44)
    return out, kinds, inert


def states(G):
    return [{"locked": g == 1, "requested_nodes": 2, "cached_cpu_m": 4000 * (g % 2), "cached_mem_b": (8 << 30) * (g % 2)}
            for g in range(G)]
