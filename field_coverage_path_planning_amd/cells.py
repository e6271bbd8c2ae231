"""Field cells: polygon fields split along a cut direction into cells that are ordinary fields, and the polygon chain run over the cells, so
that every cell is driven at its own track angle (fcpp_cells_counts / _fill; the rule: include/fcpp.h), and the cell tour: the order in
which a field's cells are driven and the route each one takes (fcpp_cell_tour_transit / _solve).  A module of its own beside engine,
whose public surface stays what it is; it uses engine's binding layer."""
import dataclasses
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from . import engine as E
from .engine import _dev_f64, _host_ptr, _one_per, _owners, _ptr, _torch, get_context

EVENTS = {'reflex': 0, 'extrema': 1}


@dataclass
class CellSet:
    """field_cells(): the cells of n fields.  Field i owns the cells cell_offsets[i] .. cell_offsets[i + 1]; cell k is field k of `fields`:
    one counter-clockwise ring."""
    fields: object              # PolygonFields: the cells, one ring per cell
    field: object               # (cells) int64: the field a cell was cut from
    cell_offsets: object        # (n + 1) int64, device; cell_offsets_host: the numpy copy
    cell_offsets_host: object
    src: object                 # (cell vertices) int32: the field-local input edge the boundary piece leaving the vertex lies on, -1: a cut leaves it
    area: object                # (cells) float64 [m^2]
    status: object              # (n) int32: 0, FCPP_EINVAL or FCPP_EUNSUPPORTED: such a field has no cells
    n_cuts: object              # (n) int32
    dropped: object             # (n) int32: the cells of at most min_area, which are not among `fields`
    dropped_area: object        # (n) float64: their summed area
    angle: object               # (n) float64: the cut angle of every field
    events: str

    @property
    def n(self):
        return int(self.cell_offsets.numel()) - 1


def field_cells(fields, cut_angle, events='extrema', min_area=0.0, device=None):
    """The decomposition (fcpp_cells_counts + fcpp_cells_fill): every field cut along `cut_angle` [rad] -- a scalar or one value per field --
    from its reflex vertices ('reflex': convex cells) or only from those where the boundary turns back across the cut direction ('extrema':
    cells that are monotone across the cuts, the boustrophedon decomposition).  Cells of at most min_area [m^2] are dropped and reported.
    `fields`: anything polygon_fields takes; rings simple and disjoint, even-odd interior, several outer rings allowed (a work area that an
    inset has split).  -> CellSet, whose .fields the swath operators, route_swaths, field_paths and polygon_coverage take as they are."""
    if events not in EVENTS:
        raise ValueError("events must be 'reflex' or 'extrema'")
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    pf = E.polygon_fields(fields, device)
    n = pf.n
    ang = _one_per(_dev_f64(cut_angle, dev), n, 'cut_angle', 'value per field')
    args = (*pf._head(), _ptr(ang), EVENTS[events], float(min_area))
    co, cvo = torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev)
    co_h, cvo_h = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    st, cuts, dropped = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    darea = torch.zeros(n, dtype=torch.float64, device=dev)
    ctx.bind_stream()
    L.check(ctx.lib.fcpp_cells_counts(ctx.handle, *args, _ptr(co), _host_ptr(co_h), _ptr(cvo), _host_ptr(cvo_h), _ptr(st), _ptr(cuts), _ptr(dropped),
                                      _ptr(darea)))
    n_cells, V = int(co_h[-1]), int(cvo_h[-1])
    ovo = torch.empty(n_cells + 1, dtype=torch.int64, device=dev)
    x, y = torch.empty(V, dtype=torch.float64, device=dev), torch.empty(V, dtype=torch.float64, device=dev)
    src, owner = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(n_cells, dtype=torch.int32, device=dev)
    area = torch.empty(n_cells, dtype=torch.float64, device=dev)
    L.check(ctx.lib.fcpp_cells_fill(ctx.handle, *args, _ptr(co), _ptr(cvo), n_cells, V, _ptr(ovo), _ptr(x), _ptr(y), _ptr(src), _ptr(owner), _ptr(area)))
    cells = E.PolygonFields(torch.arange(n_cells + 1, dtype=torch.int64, device=dev), ovo, x, y)
    return CellSet(cells, owner.to(torch.int64), co, co_h, src, area, st, cuts, dropped, darea, ang, events)


@dataclass
class CellPlan:
    """plan_polygon_cells(): every stage's result for the batch.  The stages from angle_index on are per CELL: path k is cell k's."""
    headland: object            # InsetSet: the centre lines of the headland passes
    work: object                # PolygonFields: the work areas
    cells: object               # CellSet: the work areas' cells
    angle_index: object         # (cells) int64: the chosen index into `angles`, -1 where no angle is valid
    angle: object               # (cells) float64: the track angle driven
    swaths: object              # SwathSet over the cells
    route: object               # SwathRoute
    paths: object               # FieldPaths: one path per cell
    headland_paths: object = None       # HeadlandPaths of `headland` when asked for, else None
    coverage: object = None             # PolygonCoverage of the ORIGINAL fields under the cells' paths (and the headland loops), else None
    mission: object = None              # MissionPaths: one drive per input field over its loops and its cells' paths, else None
    speeds: object = None               # PathSpeeds of `mission` when there is one, else of `paths` (speeds=vehicle), else None
    tour: object = None                 # CellTour with tour=True: the order of every field's cells and the route candidate each one drives, else None


def _cell_cover_set(paths, swaths, cells):
    """the cells' paths as polygon_coverage's tuple: the field of a path is its cell's, the swaths work, and a sample's pass id is its leg's
    slot among ALL cells' legs (leg + 2 x the cell's first swath + the cell: field_paths' own slot numbering), unique over a field's cells"""
    torch = _torch()
    total = int(paths.x.numel())
    n_cells = int(paths.offsets.numel()) - 1
    first = 2 * swaths.offsets[:-1] + torch.arange(n_cells, dtype=torch.int64, device=paths.x.device)
    owner = _owners(paths.offsets, total)
    return (paths.offsets, paths.x, paths.y, cells.field, paths.part == 0, (paths.leg.to(torch.int64) + first[owner]).to(torch.int32))


def _cell_mission_item(paths, cells):
    """the cells' paths as ONE open item set of mission_paths, in stored cell order, cells without samples left out"""
    torch = _torch()
    off_h = paths.offsets_host
    keep = np.nonzero(off_h[1:] > off_h[:-1])[0]
    off = np.concatenate([off_h[:-1][keep], [off_h[-1]]]).astype(np.int64)
    field = cells.field[torch.as_tensor(keep, device=cells.field.device)]
    return (off, paths.x, paths.y, paths.heading, paths.kappa, paths.part, paths.gear, field, False)


# ---- the cell tour (fcpp_cell_tour_transit / fcpp_cell_tour_solve; the rule: include/fcpp.h) -----------------------------------------------
TOUR_D_BUDGET = 1 << 30         # bytes of joint blocks one call of the library holds: cell_tour solves the fields in chunks below it


@dataclass
class CellTour:
    """cell_tour(): for every field the order of its cells and the node every cell takes.  Field f owns the cells cell_offsets_host[f] ..
    cell_offsets_host[f + 1]; node u = 2 v + d of a cell is its variant v, driven as given (d = 0) or backwards (d = 1)."""
    cell_offsets_host: object   # (n + 1) int64, numpy
    var_offsets_host: object    # (cells + 1) int64, numpy
    order: object               # (cells) int32, device: field-local cell indices in driving order, the cells without a variant last
    node: object                # (cells) int32: the chosen node of every cell in cell order, -1 for a cell without a variant
    cost: object                # (n) float64: inner costs plus joints (with the entry / exit joints, if given) [m]
    stored_cost: object         # (n) float64: the same for the stored order at the stored nodes
    joint_length: object        # (n) float64: the joints alone
    winner: object              # (n) int32: the candidate that gave `order`
    sweeps: object              # (n) int32: the most moves any candidate of the field applied
    skipped: object             # (n) int32: the cells without a variant
    status: object              # (n) int32: 0, FCPP_EUNSUPPORTED (beyond a cap: stored order, nodes -1, costs NaN) or FCPP_EINVAL (a non-finite stored cost)
    tours: object               # (starts, cells) int32: every candidate's final order
    costs: object               # (n, starts) float64: and its cost

    def field(self, f):
        return self.order[int(self.cell_offsets_host[f]):int(self.cell_offsets_host[f + 1])]


def _tour_block_sizes(coff_h, voff_h):
    """the entries of every field's joint block: N_f^2, none beyond a cap"""
    V = np.diff(voff_h)
    size = np.zeros(len(coff_h) - 1, dtype=np.int64)
    for f in range(len(size)):
        c0, c1 = int(coff_h[f]), int(coff_h[f + 1])
        Nf = 2 * int(voff_h[c1] - voff_h[c0])
        fits = c1 - c0 <= L.TOUR_MAX_CELLS and Nf <= L.TOUR_MAX_NODES and 2 * int(V[c0:c1].max(initial=0)) <= L.TOUR_MAX_CELL_NODES
        size[f] = Nf * Nf if fits else 0
    return size


def _tour_chunks(size, budget):
    """[lo, hi) ranges of consecutive fields whose joint blocks stay within `budget` bytes (a field alone is at most 8 MiB)"""
    out, lo, acc = [], 0, 0
    for i, b in enumerate(size * 8):
        if i > lo and acc + b > budget:
            out.append((lo, i))
            lo, acc = i, 0
        acc += int(b)
    if len(size) > lo or not out:
        out.append((lo, len(size)))
    return out


def _tour_gate(pose, own, per_field, at_entry, radius, reversing, device):
    """E (at_entry) or X: the connector length between each field's pose and every node's in-pose / from its out-pose"""
    torch = _torch()
    pose = _dev_f64(pose, own.device).reshape(-1, 3)
    if pose.shape[0] != per_field.numel():
        raise ValueError('entry / exit must hold one pose (x, y, heading) per field')
    far = torch.repeat_interleave(pose, per_field, dim=0)
    frm, to = (far, own) if at_entry else (own, far)
    return E._conn_solve_poses(frm, to, radius, reversing, device)[2].contiguous()


def cell_tour(cell_offsets, var_offsets, in_poses, out_poses, w, radius, reversing=False, entry=None, exit=None, stored_node=None, starts=8,
              min_gain=1e-9, max_sweeps=None, device=None):
    """Order of every field's cells and one node per cell (fcpp_cell_tour_transit + fcpp_cell_tour_solve; the rule: include/fcpp.h) ->
    CellTour.  Field f owns the cells cell_offsets[f] .. cell_offsets[f + 1], cell c the variants var_offsets[c] .. var_offsets[c + 1];
    in_poses / out_poses (variants, 3): where a variant is entered and left, (x, y, heading); w (variants): the price of driving it [m].
    Every variant may be driven as given or backwards (in- and out-pose swapped, headings + pi) at the same w.  The cost of a tour is the
    chosen variants' w plus the joints between consecutive cells -- shortest Dubins paths at `radius`, Reeds-Shepp if `reversing` -- plus,
    with entry / exit (one pose per field), the joints from the entry pose and to the exit pose.  For a given order the nodes are chosen
    exactly; the order is a local search: `starts` candidate orders (the stored one, its reverse, nearest-neighbour orders) are each
    improved by segment reversals and or-opt moves until none gains more than min_gain [m] (or max_sweeps moves: None = 8 x the largest
    cell count + 8); the cheapest wins.  stored_node (cells): the node that stored_cost prices in every cell (None: node 0).  Joints know
    no boundary.  Fields are solved in chunks of at most TOUR_D_BUDGET bytes of joint blocks.  A field of more than 32 cells, with a cell
    of more than 32 variants or of more than 512 variants in all keeps its stored order (status FCPP_EUNSUPPORTED)."""
    ctx = get_context(device)
    torch = _torch()
    dev = torch.device('cuda', ctx.device)
    coff_h = np.ascontiguousarray(cell_offsets.cpu().numpy() if isinstance(cell_offsets, torch.Tensor) else cell_offsets, dtype=np.int64)
    voff_h = np.ascontiguousarray(var_offsets.cpu().numpy() if isinstance(var_offsets, torch.Tensor) else var_offsets, dtype=np.int64)
    n, n_cells, n_vars = len(coff_h) - 1, len(voff_h) - 1, int(voff_h[-1])
    if n < 0 or n_cells < 0 or int(coff_h[-1]) != n_cells:
        raise ValueError('cell_offsets must hold n + 1 values that end at the number of cells')
    pin, pout = _dev_f64(in_poses, dev).reshape(-1, 3), _dev_f64(out_poses, dev).reshape(-1, 3)
    wv = _dev_f64(w, dev).reshape(-1)
    if pin.shape[0] != n_vars or pout.shape[0] != n_vars or int(wv.numel()) != n_vars:
        raise ValueError('in_poses, out_poses and w must hold one row per variant')
    cols = [p[:, k].contiguous() for p in (pin, pout) for k in range(3)]
    sn = None if stored_node is None else torch.as_tensor(stored_node, device=dev).to(torch.int32).reshape(-1).contiguous()
    if sn is not None and int(sn.numel()) != n_cells:
        raise ValueError('stored_node must hold one node per cell')
    S = int(starts)
    if max_sweeps is None:
        max_sweeps = 8 * int(np.diff(coff_h).max(initial=0)) + 8
    max_sweeps = min(int(max_sweeps), 1 << 20)
    R, mode = float(radius), 1 if reversing else 0
    nodes_per_field = torch.as_tensor(2 * (voff_h[coff_h[1:]] - voff_h[coff_h[:-1]]), device=dev)
    E_all = X_all = None
    if entry is not None or exit is not None:
        flip = torch.tensor([0.0, 0.0, np.pi], dtype=torch.float64, device=dev)
        node_in = torch.stack([pin, pout + flip], dim=1).reshape(-1, 3)           # node 2 v: the in-pose; 2 v + 1: the out-pose, heading + pi
        node_out = torch.stack([pout, pin + flip], dim=1).reshape(-1, 3)
        E_all = _tour_gate(entry, node_in, nodes_per_field, True, R, reversing, device) if entry is not None else None
        X_all = _tour_gate(exit, node_out, nodes_per_field, False, R, reversing, device) if exit is not None else None
    order, node = (torch.empty(n_cells, dtype=torch.int32, device=dev) for _ in range(2))
    tours = torch.empty((max(S, 0), n_cells), dtype=torch.int32, device=dev)
    costs = torch.empty((n, max(S, 0)), dtype=torch.float64, device=dev)
    cost, stored, joint = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
    winner, sweeps, skipped, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    size = _tour_block_sizes(coff_h, voff_h)
    ctx.bind_stream()
    for lo, hi in _tour_chunks(size, TOUR_D_BUDGET):
        c0, c1 = int(coff_h[lo]), int(coff_h[hi])
        v0, v1 = int(voff_h[c0]), int(voff_h[c1])
        co_h = np.ascontiguousarray(coff_h[lo:hi + 1] - c0)
        vo_h = np.ascontiguousarray(voff_h[c0:c1 + 1] - v0)
        do_h = np.concatenate([[0], np.cumsum(size[lo:hi])]).astype(np.int64)
        co, vo, do = (torch.as_tensor(a, device=dev) for a in (co_h, vo_h, do_h))
        d_total = int(do_h[-1])
        D = torch.empty(d_total, dtype=torch.float64, device=dev)
        head = (hi - lo, _ptr(co), _host_ptr(co_h), c1 - c0, _ptr(vo), _host_ptr(vo_h), v1 - v0)
        pc = [c[v0:v1] for c in cols]                     # (slices of contiguous columns)
        L.check(ctx.lib.fcpp_cell_tour_transit(ctx.handle, *head, *[_ptr(c) for c in pc], R, mode, _ptr(do), _host_ptr(do_h), d_total, _ptr(D)))
        Ec = E_all[2 * v0:2 * v1] if E_all is not None else None
        Xc = X_all[2 * v0:2 * v1] if X_all is not None else None
        tr = torch.empty((max(S, 0), c1 - c0), dtype=torch.int32, device=dev)
        L.check(ctx.lib.fcpp_cell_tour_solve(ctx.handle, *head, _ptr(wv[v0:v1]), _ptr(sn[c0:c1]) if sn is not None else _ptr(None), _ptr(do),
                                             _host_ptr(do_h), d_total, _ptr(D), _ptr(Ec), _ptr(Xc), S, float(min_gain), max_sweeps,
                                             _ptr(order[c0:c1]), _ptr(node[c0:c1]), _ptr(cost[lo:hi]), _ptr(stored[lo:hi]), _ptr(joint[lo:hi]),
                                             _ptr(winner[lo:hi]), _ptr(sweeps[lo:hi]), _ptr(skipped[lo:hi]), _ptr(status[lo:hi]), _ptr(tr),
                                             _ptr(costs[lo:hi])))
        tours[:, c0:c1] = tr
    return CellTour(coff_h, voff_h, order, node, cost, stored, joint, winner, sweeps, skipped, status, tours, costs)


def _tour_variants(ss, route):
    """every cell's variants from its router candidates -> (var_offsets numpy, in_poses, out_poses, w, stored_node): a cell whose route
    status is 0 gets one variant per candidate c -- the start of the first oriented swath of route.tours[c] and the end of the last one,
    headings as SwathSet.poses has them, w = route.costs[cell, c]; any other cell with swaths gets route.order at w = 0; a cell without
    swaths gets none"""
    torch = _torch()
    dev = ss.a.device
    soff_h = np.asarray(ss.offsets_host, dtype=np.int64)
    m = np.diff(soff_h)
    S = int(route.tours.shape[0])
    ok_h = route.status.cpu().numpy() == 0
    V = np.where(m == 0, 0, np.where(ok_h, S, 1)).astype(np.int64)
    voff_h = np.concatenate([[0], np.cumsum(V)]).astype(np.int64)
    n_cells, n_vars = len(m), int(voff_h[-1])
    voff = torch.as_tensor(voff_h, device=dev)
    vc = _owners(voff, n_vars)                                   # the cell of every variant
    vk = torch.arange(n_vars, dtype=torch.int64, device=dev) - voff[vc]      # and its candidate
    ok = torch.as_tensor(ok_h, device=dev)[vc]
    first, last = ss.offsets[vc], ss.offsets[vc + 1] - 1
    order = route.order.to(torch.int64)
    tours = route.tours.to(torch.int64)
    p0 = torch.where(ok, tours[vk, first], order[first]) if n_vars else first
    p1 = torch.where(ok, tours[vk, last], order[last]) if n_vars else last
    th = ss.angle[vc]
    flipped = th + np.pi

    def pose(p, leaving):
        g, d = ss.offsets[vc] + (p >> 1), (p & 1) == 1
        at_b = d != leaving                                      # d = 0 starts at a and ends at b, d = 1 the other way
        xy = torch.where(at_b.unsqueeze(1), ss.b[g], ss.a[g])
        return torch.cat([xy, torch.where(d, flipped, th).unsqueeze(1)], dim=1)

    w = torch.where(ok, route.costs[vc, vk], torch.zeros((), dtype=torch.float64, device=dev)) if n_vars else torch.zeros(0, dtype=torch.float64, device=dev)
    return voff_h, pose(p0, False), pose(p1, True), w, (2 * route.winner).to(torch.int32)


def _tour_route(ss, route, tour):
    """the route with every cell's driven order as its chosen node has it: the candidate tour as it is for d = 0, reversed with every
    member flipped for d = 1; a cell without a node keeps route.order"""
    torch = _torch()
    dev = ss.a.device
    total = int(ss.offsets_host[-1])
    cell = _owners(ss.offsets, total)
    node = tour.node.to(torch.int64)
    took = (node >= 0) & (route.status == 0)
    cand = torch.where(took, node >> 1, torch.zeros_like(node))
    back = (node >= 0) & ((node & 1) == 1)
    at = torch.arange(total, dtype=torch.int64, device=dev)
    src = torch.where(back[cell], ss.offsets[cell] + ss.offsets[cell + 1] - 1 - at, at)
    base = torch.where(took[cell], route.tours.to(torch.int64)[cand[cell], src], route.order.to(torch.int64)[src]) if total else at
    order = (base ^ back[cell].to(torch.int64)).to(torch.int32).contiguous()
    cost = torch.where(took, route.costs[torch.arange(int(node.numel()), device=dev), cand], route.cost)
    return dataclasses.replace(route, order=order, cost=cost, winner=torch.where(took, cand.to(torch.int32), route.winner))


@dataclass
class CellPaths(E.PathSet):
    """the cells' paths as ONE open item set of mission_paths, driven in the cell tour's order: path k is cell k's"""
    cell_field: object = None   # (cells) int64: the field of every cell
    order: object = None        # (driven cells) int64: the cells with samples, field by field in the tour's order

    def path_field(self):
        return self.cell_field

    def drive_order(self, innermost_first=False):
        return self.order


def _cell_tour_item(paths, cells, tour):
    """the cells' paths as a CellPaths: every field's cells in tour.order, cells without samples left out"""
    torch = _torch()
    dev = paths.x.device
    coff = torch.as_tensor(tour.cell_offsets_host, device=dev)
    n_cells = int(tour.cell_offsets_host[-1])
    order = tour.order.to(torch.int64) + coff[:-1][_owners(coff, n_cells)]
    has = torch.as_tensor(paths.offsets_host[1:] > paths.offsets_host[:-1], device=dev)
    return CellPaths(paths.offsets, paths.offsets_host, paths.x, paths.y, paths.heading, paths.kappa, paths.part, paths.gear, cells.field.to(torch.int64),
                     order[has[order]].contiguous())


def plan_polygon_cells(fields, width, radius, spacing, angles, cut_angle, events='extrema', min_cell_area=None, passes=1, turn_cost=0.0,
                       reversing=False, starts=8, entry=None, exit=None, arc_step=0.1, headland_paths=False, coverage_resolution=None,
                       mission=None, speeds=None, device=None, tour=False):
    """The polygon chain with an angle per CELL, every stage one batched call on the device: headland(passes) -> field_cells of the work areas
    along cut_angle (min_cell_area: default width^2) -> best_swath_angle over `angles`, polygon_swaths, route_swaths(spacing=spacing) and
    field_paths over the cells.  -> CellPlan.  A cell for which no angle is valid carries its stage's status and has no samples.
    headland_paths=True also drives the pass rings (one closed loop per ring).  coverage_resolution [m]: what the plan covers of the ORIGINAL
    fields (polygon_coverage; the cells' paths count for their field, pass ids unique over a field's cells).  Adjacent cells driven at
    different angles leave wedges at their seams, which no headland pass covers: the report shows them.
    mission='headland_first' | 'headland_last' (with headland_paths=True; ValueError without): ONE drive per input field (mission_paths):
    its loops and its cells' paths, the cells in stored order, cells without samples left out.  entry / exit, one pose per input field,
    belong to the mission (ValueError without one: a cell has no gate of its own).  speeds=vehicle: path_speeds of the mission when there
    is one, else of the cells' paths.  The chain offers no clearance, reshape, detour or patch: those stay with plan_polygon_fields.
    tour=True: the cell tour (cell_tour) decides the order of every field's cells and, per cell, which of the router's `starts` candidate
    routes is driven and in which direction, so that the candidates' costs plus the joints between cells -- and to the mission's exit
    pose under 'headland_first', from its entry pose under 'headland_last' -- are least; CellPlan.tour holds the result, .route the routes
    as driven, and the mission drives the cells in the tour's order.  Without it nothing changes, down to the entries called."""
    if mission not in (None, 'headland_first', 'headland_last'):
        raise ValueError("mission must be None, 'headland_first' or 'headland_last'")
    if mission is not None and not headland_paths:
        raise ValueError('mission needs headland_paths=True: the loops the mission drives')
    if mission is None and (entry is not None or exit is not None):
        raise ValueError('entry / exit need mission=...: they are the gates of the field, not of a cell')
    torch = _torch()
    fields = E.polygon_fields(fields, device)
    lines, work = E.headland(fields, width, passes, arc_step=arc_step, device=device)
    cells = field_cells(work, cut_angle, events, float(width) ** 2 if min_cell_area is None else float(min_cell_area), device=device)
    cf = cells.fields
    ang = _dev_f64(angles, cf.x.device).reshape(-1)
    idx, _ = E.best_swath_angle(cf, ang, width, turn_cost, device=device)
    chosen = ang[idx.clamp(min=0)] if ang.numel() else torch.zeros(cf.n, dtype=torch.float64, device=cf.x.device)
    ss = E.polygon_swaths(cf, chosen, width, device=device)
    route = E.route_swaths(ss, radius, reversing=reversing, starts=starts, spacing=spacing, device=device)
    hp = E.headland_paths(lines, radius, spacing, reversing=reversing, device=device) if headland_paths else None
    ct = None
    if tour:
        voff_h, pin, pout, w, stored_node = _tour_variants(ss, route)
        ct = cell_tour(cells.cell_offsets_host, voff_h, pin, pout, w, E._chord_radius(radius, spacing), reversing=reversing,
                       entry=entry if mission == 'headland_last' else None, exit=exit if mission == 'headland_first' else None,
                       stored_node=stored_node, starts=starts, device=device)
        route = _tour_route(ss, route, ct)
    paths = E.field_paths(ss, radius, spacing, reversing=reversing, order=route, device=device)
    plan = CellPlan(lines, work, cells, idx, chosen, ss, route, paths, hp, tour=ct)
    if coverage_resolution is not None:
        as_set = _cell_cover_set(paths, ss, cells)
        plan.coverage = E.polygon_coverage(fields, width, coverage_resolution, paths=(as_set,) if hp is None else (as_set, hp), device=device)
    if mission is not None:
        item = _cell_mission_item(paths, cells) if ct is None else _cell_tour_item(paths, cells, ct)
        plan.mission = E.mission_paths((hp, item) if mission == 'headland_first' else (item, hp), radius, spacing, reversing=reversing, entry=entry,
                                       exit=exit, device=device, innermost_first=mission == 'headland_last', n_fields=fields.n)
    if speeds is not None:
        plan.speeds = E.path_speeds(plan.mission if plan.mission is not None else paths, speeds, device=device)
    return plan
