"""Field cells: polygon fields split along a cut direction into cells that are ordinary fields, and the polygon chain run over the cells, so
that every cell is driven at its own track angle (fcpp_cells_counts / _fill; the rule: include/fcpp.h).  A module of its own beside
engine, whose public surface stays what it is; it uses engine's binding layer."""
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


def plan_polygon_cells(fields, width, radius, spacing, angles, cut_angle, events='extrema', min_cell_area=None, passes=1, turn_cost=0.0,
                       reversing=False, starts=8, entry=None, exit=None, arc_step=0.1, headland_paths=False, coverage_resolution=None,
                       mission=None, speeds=None, device=None):
    """The polygon chain with an angle per CELL, every stage one batched call on the device: headland(passes) -> field_cells of the work areas
    along cut_angle (min_cell_area: default width^2) -> best_swath_angle over `angles`, polygon_swaths, route_swaths(spacing=spacing) and
    field_paths over the cells.  -> CellPlan.  A cell for which no angle is valid carries its stage's status and has no samples.
    headland_paths=True also drives the pass rings (one closed loop per ring).  coverage_resolution [m]: what the plan covers of the ORIGINAL
    fields (polygon_coverage; the cells' paths count for their field, pass ids unique over a field's cells).  Adjacent cells driven at
    different angles leave wedges at their seams, which no headland pass covers: the report shows them.
    mission='headland_first' | 'headland_last' (with headland_paths=True; ValueError without): ONE drive per input field (mission_paths):
    its loops and its cells' paths, the cells in stored order, cells without samples left out.  entry / exit, one pose per input field,
    belong to the mission (ValueError without one: a cell has no gate of its own).  speeds=vehicle: path_speeds of the mission when there
    is one, else of the cells' paths.  The chain offers no clearance, reshape, detour or patch: those stay with plan_polygon_fields."""
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
    paths = E.field_paths(ss, radius, spacing, reversing=reversing, order=route, device=device)
    plan = CellPlan(lines, work, cells, idx, chosen, ss, route, paths, hp)
    if coverage_resolution is not None:
        as_set = _cell_cover_set(paths, ss, cells)
        plan.coverage = E.polygon_coverage(fields, width, coverage_resolution, paths=(as_set,) if hp is None else (as_set, hp), device=device)
    if mission is not None:
        item = _cell_mission_item(paths, cells)
        plan.mission = E.mission_paths((hp, item) if mission == 'headland_first' else (item, hp), radius, spacing, reversing=reversing, entry=entry,
                                       exit=exit, device=device, innermost_first=mission == 'headland_last', n_fields=fields.n)
    if speeds is not None:
        plan.speeds = E.path_speeds(plan.mission if plan.mission is not None else paths, speeds, device=device)
    return plan
