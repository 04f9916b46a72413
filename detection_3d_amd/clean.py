"""Cleaning a raw scan before it is voxelised.  voxelize puts the origin at the cloud's per-axis minimum and drops what
leaves the lattice, so one lidar return through a window, a flying pixel of fuse_frames or a detached blob 60 m away
moves the origin and can push half the building out.  The reference only works round it (check_points_out_of_house
throws the whole frame away, data3d/suncg_utils/suncg_preprocess.py:721-732; crop_special_scenes crops by hand,
data3d/indoor_data_util.py:339); its users call open3d's remove_radius_outlier, remove_statistical_outlier and a
clustering pass on the CPU.  Here the three are calls on the GPU (libd3d_hip, clean.hip), consumers of the cell list
that estimate_normals builds.

Semantics (include/d3d_hip.h), restatements that are not pinned against open3d itself: "within radius" is
estimate_normals' test, d2 = (dx dx + dy dy) + dz dz <= radius^2 in fp32, the point itself included.
radius_outliers keeps a point with at least min_neighbors points within radius (itself counted, where open3d's count
leaves it out).  statistical_outliers is open3d's remove_statistical_outlier on a hybrid search: the k nearest
neighbours within radius by (d2, index), their mean distance in fp64, the mean and the sample deviation of those means
over the points that have k neighbours; a point with fewer is dropped and enters neither.  connected_components labels
the graph whose edges join points within radius.  The same input gives the same bits, whatever torch's deterministic
mode says."""
import torch

from ._cloud import PhaseTimer, gpu_rows, number, options, run, scratch, whole
from ._lib import ptr, stream_of

PHASES = ("cells", "sort", "table", "search", "tail")


def _check_statistical(statistical):
    try:
        k, std_ratio = statistical
    except (TypeError, ValueError):
        raise ValueError(f"statistical must be None or (k, std_ratio), got {statistical!r}") from None
    return whole(k, "statistical: k"), number(std_ratio, "statistical: std_ratio")


def _check_min_component(min_component):
    """an int >= 1 (points), or a float in (0, 1) (a share of the rows given to the step)"""
    if isinstance(min_component, bool):
        raise ValueError(f"min_component {min_component!r} must be an int >= 1 or a float in (0, 1)")
    if isinstance(min_component, int):
        if min_component < 1:
            raise ValueError(f"min_component {min_component} < 1")
        return min_component
    if isinstance(min_component, float):
        if not 0.0 < min_component < 1.0:
            raise ValueError(f"min_component {min_component}: a share lies in (0, 1); give a number of points as an int")
        return min_component
    raise ValueError(f"min_component {min_component!r} must be an int >= 1 or a float in (0, 1)")


def radius_neighbors(xyz, radius=0.1, phases=False):
    """xyz fp32 [N, >= 3] on the GPU (a column slice of a wider cloud is read in place) -> count int32 [N], the points
    within `radius` of every point, itself included.  Current stream, no read-back.  phases: also a dict of milliseconds
    (PHASES), timed with events inside the library; synchronises."""
    radius = number(radius, "radius", lo_open=True)
    xyz, n, stride = gpu_rows(xyz)
    dev = xyz.device
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    timer = PhaseTimer(PHASES, phases)
    if n > 0:
        buf, nbytes = scratch(dev, "d3d_radius_neighbors_scratch_bytes", n)
        run(dev, "d3d_radius_neighbors", ptr(xyz), n, stride, radius, ptr(count), ptr(buf), nbytes, stream_of(dev),
            timer.ms)
    return (count, timer.read()) if phases else count


def radius_outliers(xyz, radius=0.1, min_neighbors=8, return_counts=False):
    """-> keep bool [N]: the point has at least min_neighbors points within radius, itself counted; with return_counts
    also those counts, int32 [N]."""
    min_neighbors = whole(min_neighbors, "min_neighbors")
    count = radius_neighbors(xyz, radius)
    keep = count >= min_neighbors
    return (keep, count) if return_counts else keep


def knn_mean_distance(xyz, k=20, std_ratio=2.0, radius=0.1, phases=False):
    """-> (mean fp64 [N], found int32 [N], stats fp64 [2] = (mu, sigma) on the device, keep bool [N]) of
    d3d_knn_mean_distance; phases: also the dict of milliseconds (synchronises)."""
    radius = number(radius, "radius", lo_open=True)
    k, std_ratio = _check_statistical((k, std_ratio))
    xyz, n, stride = gpu_rows(xyz)
    dev = xyz.device
    mean = torch.empty((n,), dtype=torch.float64, device=dev)
    found = torch.empty((n,), dtype=torch.int32, device=dev)
    keep = torch.empty((n,), dtype=torch.bool, device=dev)
    stats = torch.empty((2,), dtype=torch.float64, device=dev)
    timer = PhaseTimer(PHASES, phases)
    buf, nbytes = scratch(dev, "d3d_knn_mean_distance_scratch_bytes", n)
    run(dev, "d3d_knn_mean_distance", ptr(xyz), n, stride, radius, k, std_ratio, ptr(mean), ptr(found), ptr(stats),
        ptr(keep), ptr(buf), nbytes, stream_of(dev), timer.ms)
    res = (mean, found, stats, keep)
    return res + (timer.read(),) if phases else res


def statistical_outliers(xyz, k=20, std_ratio=2.0, radius=0.1, return_stats=False):
    """open3d's remove_statistical_outlier on a hybrid search; a restatement that is not pinned against open3d itself.
    The neighbours of a point are its k nearest within `radius` by (squared distance, index); its mean distance to them
    is taken in fp64; mu and sigma are the mean and the sample deviation (division by count - 1) of those means over the
    points that have k neighbours.  -> keep bool [N]: the point has k neighbours and mean <= mu + std_ratio sigma.  A
    point with fewer than k neighbours within radius is dropped and enters neither mu nor sigma (its mean is +inf).
    return_stats: -> (keep, the means fp64 [N], a 2-element device tensor (mu, sigma)).  Current stream, no read-back."""
    mean, _, stats, keep = knn_mean_distance(xyz, k, std_ratio, radius)
    return (keep, mean, stats) if return_stats else keep


def connected_components(xyz, radius=0.1, phases=False):
    """The components of the graph whose edges join points within `radius` of one another -> (label int32 [N], the
    smallest row index of the point's component; size int32 [N], that component's number of points).  Current stream,
    no read-back."""
    radius = number(radius, "radius", lo_open=True)
    xyz, n, stride = gpu_rows(xyz)
    dev = xyz.device
    label = torch.empty((n,), dtype=torch.int32, device=dev)
    size = torch.empty((n,), dtype=torch.int32, device=dev)
    timer = PhaseTimer(PHASES, phases)
    if n > 0:
        buf, nbytes = scratch(dev, "d3d_connected_components_scratch_bytes", n)
        run(dev, "d3d_connected_components", ptr(xyz), n, stride, radius, ptr(label), ptr(size), ptr(buf), nbytes,
            stream_of(dev), timer.ms)
    return (label, size, timer.read()) if phases else (label, size)


def component_threshold(min_component, rows):
    """the number of points a component needs: an int as it is, a float in (0, 1) as that share of `rows`"""
    return min_component if isinstance(min_component, int) else min_component * rows


def compose_sources(first, second):
    """Two source maps in a row (row of the input -> row of the result, -1 for a dropped row; either may be None, the
    identity) -> the map from the first step's input to the second step's result."""
    if first is None:
        return second
    if second is None:
        return first
    # entry M of the table: the rows the first step dropped (source -1 indexes it from the end)
    table = torch.cat([second, torch.full((1,), -1, dtype=second.dtype, device=second.device)])
    return table[first.long()]


def _compact(pcl, keep, source):
    """the kept rows in their order, every column; source: the map so far, or None while it is not wanted"""
    out = pcl[keep]                                    # the step's one size read-back
    if source is not None:
        new_row = torch.cumsum(keep, 0, dtype=torch.int32) - 1
        new_row = torch.where(keep, new_row, torch.full_like(new_row, -1))
        source = compose_sources(source, new_row)
    return out, source


def clean_cloud(pcl, radius=0.1, min_neighbors=None, statistical=None, min_component=None, return_source=False):
    """pcl fp32 [N, C >= 3] on the GPU, columns 0:3 the position -> its rows that pass the steps whose option is set, in
    the fixed order radius_outliers(min_neighbors) -> statistical_outliers(*statistical), statistical = (k, std_ratio)
    -> connected_components with min_component: an int (points) or a float in (0, 1) (a share of the rows given to that
    step); a component stays when its size >= that number.  Each step runs on the survivors of the one before; the row
    order and every column are kept.  One size read-back per step.  With every option None the result is `pcl` itself and
    no kernel is issued.
    return_source: also source int32 [N], the row of the result every input row went to, -1 for a dropped row (None when
    every option is None)."""
    kw = clean_kwargs({"radius": radius, "min_neighbors": min_neighbors, "statistical": statistical,
                       "min_component": min_component})
    radius, min_neighbors, statistical, min_component = (kw.get(k) for k in _CLEAN_KEYS)
    if min_neighbors is None and statistical is None and min_component is None:
        return (pcl, None) if return_source else pcl
    if not isinstance(pcl, torch.Tensor) or pcl.dim() != 2 or pcl.shape[1] < 3:
        raise ValueError("clean_cloud: a tensor [N, >= 3]")
    source = torch.arange(pcl.shape[0], dtype=torch.int32, device=pcl.device) if return_source else None
    if min_neighbors is not None:
        pcl, source = _compact(pcl, radius_outliers(pcl[:, :3], radius, min_neighbors), source)
    if statistical is not None:
        pcl, source = _compact(pcl, statistical_outliers(pcl[:, :3], statistical[0], statistical[1], radius), source)
    if min_component is not None:
        _, size = connected_components(pcl[:, :3], radius)
        pcl, source = _compact(pcl, size >= component_threshold(min_component, pcl.shape[0]), source)
    return (pcl, source) if return_source else pcl


_CLEAN_KEYS = ("radius", "min_neighbors", "statistical", "min_component")


def clean_kwargs(clean):
    """The `clean=` keyword of the loops: None -> None; a dict with keys among radius, min_neighbors, statistical,
    min_component (clean_cloud's keywords) -> a checked copy.  Unknown keys and bad values raise ValueError."""
    clean = options(clean, "clean", _CLEAN_KEYS)
    if clean is None:
        return None
    kw = {"radius": number(clean.get("radius", 0.1), "radius", lo_open=True)}
    if clean.get("min_neighbors") is not None:
        kw["min_neighbors"] = whole(clean["min_neighbors"], "min_neighbors")
    if clean.get("statistical") is not None:
        kw["statistical"] = _check_statistical(clean["statistical"])
    if clean.get("min_component") is not None:
        kw["min_component"] = _check_min_component(clean["min_component"])
    return kw


def parse_clean(spec):
    """--clean SPEC: None or '' -> None; otherwise comma-separated KEY=VALUE with the keys radius=R, neighbors=M
    (min_neighbors), statistical=K:RATIO and component=C (min_component: an integer number of points, or a share with a
    decimal point), e.g. 'radius=0.1,neighbors=8,statistical=20:2.0,component=0.01'."""
    if spec is None or not spec.strip():
        return None
    kw = {}
    for part in spec.strip().split(","):
        name, eq, value = part.partition("=")
        name, value = name.strip(), value.strip()
        if not eq or not value:
            raise ValueError(f"--clean takes KEY=VALUE[,KEY=VALUE...], got {part!r} in {spec!r}")
        if name in kw or {"neighbors": "min_neighbors", "component": "min_component"}.get(name, name) in kw:
            raise ValueError(f"--clean: {name} given twice in {spec!r}")
        try:
            if name == "radius":
                kw["radius"] = float(value)
            elif name == "neighbors":
                kw["min_neighbors"] = int(value)
            elif name == "statistical":
                k, colon, ratio = value.partition(":")
                if not colon:
                    raise ValueError("K:RATIO")
                kw["statistical"] = (int(k), float(ratio))
            elif name == "component":
                kw["min_component"] = int(value) if value.lstrip("+-").isdigit() else float(value)
            else:
                raise KeyError(name)
        except KeyError:
            raise ValueError(f"--clean: unknown key {name!r} (radius, neighbors, statistical, component)")
        except ValueError:
            raise ValueError(f"--clean: bad value {value!r} for {name}")
    return clean_kwargs(kw)


def apply_clean(pcl, ckw, return_source=False):
    """The cleaning steps of a checked `clean=` (clean_kwargs) on one cloud, on the current stream.  return_source: also
    source int32 [N] as clean_cloud gives it (None when ckw is None or sets no step)."""
    if ckw is None:
        return (pcl, None) if return_source else pcl
    return clean_cloud(pcl, return_source=return_source, **ckw)
