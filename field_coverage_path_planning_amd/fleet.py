"""Vehicle shares: a routed field divided among K vehicles of one depot so that the vehicle that finishes last finishes as early as possible,
and every vehicle's share driven as a path of its own (fcpp_fleet_solve; the rule: include/fcpp.h).  A module of its own beside engine,
whose public surface stays what it is; it uses engine's binding layer, the helpers route_swaths itself prices its connectors with, and the
regrouping of swath records the service trips drive their trips with."""
import dataclasses
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from . import engine as E
from .engine import _dev_f64, _host_ptr, _one_per, _owners, _ptr, _torch, get_context
from .trips import _gather_fields, _poses, _regrouped, _transit_chunks

MAX_VEHICLES = 16          # FCPP_FLEET_MAX_VEHICLES


@dataclass
class FleetSplit:
    """vehicle_shares(): for every field the tour that is driven and which vehicle drives which stretch of it.  Field i owns the positions
    offsets_host[i] .. offsets_host[i + 1] of `tour` and `share` (the SwathSet's offsets) and the shares share_offsets_host[i] ..
    share_offsets_host[i + 1]; share k owns the positions share_swath_offsets[k] .. share_swath_offsets[k + 1] of `tour`."""
    offsets_host: object        # (n + 1) int64, numpy
    tour: object                # (m) int32, device: oriented swaths 2 s + d in driving order, as SwathRoute.order holds them
    share: object               # (m) int32: per tour position the vehicle's index within the field, from 0, never decreasing
    n_used: object              # (n) int32: the shares used, at most min(vehicles, swaths): a vehicle that would only make things worse stays home
    winner: object              # (n) int32: the variant 2 c + r that gave `tour`: candidate c, r = 1 driven backwards
    status: object              # (n) int32: 0, FCPP_EUNSUPPORTED (more than 512 swaths, more than 16 vehicles) or FCPP_EINVAL: candidate 0 as one share, NaN costs
    makespan: object            # (n) float64: the largest share cost [m of driving]: transit + work_weight * work
    total: object               # (n) float64: the summed share costs, the least among the splits of that makespan
    makespans: object           # (n, 2 C) float64: every variant's makespan, NaN for the backward ones with both_ways=False
    totals: object              # (n, 2 C) float64: every variant's sum
    share_first: object         # (n, k_stride) int32: a share's first position in the field's tour, -1 beyond n_used
    share_cost: object          # (n, k_stride) float64: a share's cost, NaN beyond n_used
    share_offsets: object       # (n + 1) int64, device; share_offsets_host: the numpy copy
    share_offsets_host: object
    share_swath_offsets: object  # (shares + 1) int64, device: into `tour`
    share_field: object         # (shares) int64: the field of every share
    share_work: object          # (shares) float64: the summed swath length of every share [m]
    depot: object               # (n, 3) float64: the depot pose of every field
    vehicles: object            # (n) int32
    work_weight: float = 1.0    # a metre of work in metres of driving: transit speed / working speed
    makespan_s: object = None   # (n) float64: the makespan in seconds, where speeds were given
    share_time_s: object = None  # (n, k_stride) float64: every share's time in seconds

    def field(self, i):
        """(tour, share) of field i"""
        sl = slice(int(self.offsets_host[i]), int(self.offsets_host[i + 1]))
        return self.tour[sl], self.share[sl]

    def costs_per_share(self):
        """share_cost as one value per share of the CSR table: (shares) float64"""
        index = _torch().arange(int(self.share_offsets_host[-1]), dtype=_torch().int64, device=self.share_field.device) - self.share_offsets[self.share_field]
        return self.share_cost[self.share_field, index]


def vehicle_shares(swathset, route, depot, vehicles, radius, spacing=None, reversing=False, work_speed=None, transit_speed=None, candidates='all',
                   both_ways=True, clear_of=None, price_clear=False, blocked_penalty=1.0e6, device=None):
    """Which vehicle drives which stretch of a routed field (fcpp_fleet_solve; the rule: include/fcpp.h) -> FleetSplit.  `route` is the
    SwathRoute of `swathset`; depot: one pose (x, y, heading) per field, where every vehicle starts and ends; vehicles: how many there are
    (a scalar or one value per field, 1 .. 16).  A vehicle drives a contiguous stretch of the tour, from the depot and back; its cost is
    its connectors' length plus work_weight times its swaths' length, work_weight = transit_speed / work_speed [m/s] (1.0 when both are
    None), so that the cost is the vehicle's time in metres of driving.  The split is the one whose largest cost -- the makespan -- is
    least, exactly, and among those the one of least summed cost; it uses AT MOST `vehicles` shares.  candidates='all' divides every
    candidate tour the router kept (route.tours), 'route' only route.order; both_ways=True also divides each one driven backwards; the
    least (makespan, sum) wins (FleetSplit.winner).
    Transits and the ways to and from the depot are priced as route_swaths prices them -- pass the same radius, spacing, reversing,
    clear_of, price_clear and blocked_penalty -- so a share's connectors cost what share_paths drives.  Fields are solved in route_swaths'
    chunks of at most ROUTE_T_BUDGET bytes of transit blocks.  A field of more than 512 swaths or more than 16 vehicles, or with fewer
    than one, is one share over route's candidate 0 (status FCPP_EUNSUPPORTED / FCPP_EINVAL)."""
    if candidates not in ('all', 'route'):
        raise ValueError("candidates must be 'all' or 'route'")
    if price_clear and clear_of is None:
        raise ValueError('price_clear=True needs clear_of: the region the connectors have to stay clear of')
    if (work_speed is None) != (transit_speed is None):
        raise ValueError('work_speed and transit_speed are given together or not at all')
    omega = 1.0 if work_speed is None else float(transit_speed) / float(work_speed)
    if not (omega >= 0.0 and np.isfinite(omega)) or (transit_speed is not None and not float(transit_speed) > 0.0):
        raise ValueError('work_speed and transit_speed must be positive and finite')
    ctx = get_context(device)
    torch = _torch()
    ss = swathset
    dev = ss.a.device
    R = float(radius) if spacing is None else E._chord_radius(radius, spacing)
    soff_all = np.asarray(ss.offsets_host, dtype=np.int64)
    n, m_total = len(soff_all) - 1, int(soff_all[-1])
    dep = _poses(depot, n, dev, 'depot')
    Kf = _one_per(torch.as_tensor(np.asarray(vehicles.cpu() if isinstance(vehicles, torch.Tensor) else vehicles), device=dev).to(torch.int32), n,
                  'vehicles', 'value per field').contiguous()
    k_stride = min(max(int(Kf.max()) if n else 1, 1), MAX_VEHICLES)
    tours = (route.tours if candidates == 'all' else route.order.reshape(1, -1)).to(torch.int32)
    C = int(tours.shape[0])
    if int(tours.shape[1]) != m_total:
        raise ValueError('route must be the SwathRoute of the SwathSet')
    pf = None if clear_of is None else E._clear_fields(clear_of, n, device)
    ends = lambda at_entry: E._route_ends(ss, dep, at_entry, R, reversing, device, pf, blocked_penalty, price_clear)
    In_all, Out_all = ends(True), ends(False)
    tour, share = (torch.empty(m_total, dtype=torch.int32, device=dev) for _ in range(2))
    n_used, winner, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    makespan, total = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    makespans, totals = (torch.empty((n, 2 * C), dtype=torch.float64, device=dev) for _ in range(2))
    share_first = torch.empty((n, k_stride), dtype=torch.int32, device=dev)
    share_cost = torch.empty((n, k_stride), dtype=torch.float64, device=dev)
    for lo, hi, ch, T in _transit_chunks(ctx, ss, R, reversing, pf, blocked_penalty, price_clear):
        s0, m = int(soff_all[lo]), ch.m
        part = lambda a: a[2 * s0:2 * (s0 + m)]
        tr = tours[:, s0:s0 + m].contiguous()
        ctx.bind_stream()
        L.check(ctx.lib.fcpp_fleet_solve(ctx.handle, hi - lo, _ptr(ch.soff), _host_ptr(ch.soff_h), m, _ptr(ch.toff), _host_ptr(ch.toff_h),
                                         int(ch.toff_h[-1]), _ptr(T), _ptr(ss.length[s0:s0 + m]), _ptr(part(In_all)), _ptr(part(Out_all)), C, _ptr(tr),
                                         1 if both_ways else 0, _ptr(Kf[lo:hi]), k_stride, omega, _ptr(tour[s0:s0 + m]), _ptr(share[s0:s0 + m]),
                                         _ptr(n_used[lo:hi]), _ptr(winner[lo:hi]), _ptr(status[lo:hi]), _ptr(makespan[lo:hi]), _ptr(total[lo:hi]),
                                         _ptr(makespans[lo:hi]), _ptr(totals[lo:hi]), _ptr(share_first[lo:hi]), _ptr(share_cost[lo:hi])))
    # the shares as a CSR table over the tour
    nu_h = n_used.cpu().numpy().astype(np.int64)
    hoff_h = np.concatenate([[0], np.cumsum(nu_h)]).astype(np.int64)
    hoff = torch.as_tensor(hoff_h, device=dev)
    S = int(hoff_h[-1])
    field_of = _owners(ss.offsets, m_total)
    global_share = share.to(torch.int64) + hoff[:-1][field_of]
    per_share = torch.bincount(global_share, minlength=S) if m_total else torch.zeros(S, dtype=torch.int64, device=dev)
    hso = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(per_share, 0)])
    swath = ss.offsets[field_of] + (tour.to(torch.int64) >> 1)
    work = torch.zeros(S, dtype=torch.float64, device=dev).index_add_(0, global_share, ss.length[swath])
    # (a tensor of the speed, not the scalar: a division by a scalar is a product with its rounded reciprocal on the device)
    seconds = (None, None) if transit_speed is None else (makespan / torch.full_like(makespan, float(transit_speed)),
                                                          share_cost / torch.full_like(share_cost, float(transit_speed)))
    return FleetSplit(soff_all, tour, share, n_used, winner, status, makespan, total, makespans, totals, share_first, share_cost, hoff, hoff_h, hso,
                      _owners(hoff, S), work, dep, Kf, omega, *seconds)


@dataclass
class SharePaths(E.FieldPaths):
    """share_paths(): one sampled path per SHARE: a FieldPaths whose path k is share k's -- one vehicle's drive, depot to depot -- over
    `swaths`, the SwathSet whose "fields" are the shares."""
    swaths: object = None       # SwathSet: the swath records regrouped by share, in driving order
    share_field: object = None  # (shares) int64: the field of every share
    share_first: object = None  # (shares) int64: the share's first position within its field's tour
    share_index: object = None  # (shares) int64: the share's index within its field: the vehicle

    def path_field(self):
        return self.share_field

    def pass_id(self):
        """the leg's slot as the undivided path of the same tour numbers it, moved on by the share's index: unique over a field's shares"""
        owner = _owners(self.offsets, int(self.x.numel()))
        return (self.leg.to(_torch().int64) + (2 * self.share_first + self.share_index)[owner]).to(_torch().int32)


def share_paths(swathset, split, radius, spacing, reversing=False, clear_of=None, device=None):
    """Every share of a FleetSplit as a sampled path (field_paths over the shares) -> SharePaths.  The swath records are regrouped by share
    into a SwathSet whose "fields" are the shares (SharePaths.swaths), as trip_paths regroups them by trip, and field_paths drives each one
    in the tour's order and directions, from the field's depot pose and back to it.  clear_of (one region per field of `swathset`): every
    share's connectors drive the shortest word that stays off its field's region (field_paths(clear_of=...)).  path_speeds, trajectory,
    validate and polygon_coverage take the result as they take any path set; every vehicle stands at both ends of its share."""
    torch = _torch()
    ss = swathset
    dev = ss.a.device
    S = int(split.share_offsets_host[-1])
    sf = split.share_field
    hso = split.share_swath_offsets
    shares, order = _regrouped(ss, split.tour, hso, sf)
    index = torch.arange(S, dtype=torch.int64, device=dev) - split.share_offsets[sf]
    first = hso[:-1] - ss.offsets[sf]
    dep = split.depot[sf]
    region = None
    if clear_of is not None:
        region = _gather_fields(E._clear_fields(clear_of, len(split.offsets_host) - 1, device), sf.cpu().numpy())
    fp = E.field_paths(shares, radius, spacing, reversing=reversing, order=order, entry=dep, exit=dep, device=device, clear_of=region)
    return SharePaths(**{f.name: getattr(fp, f.name) for f in dataclasses.fields(fp)}, swaths=shares, share_field=sf, share_first=first, share_index=index)


def plan_fleet(plan, depot, vehicles, radius, spacing, reversing=False, clear_of=None, device=None, **kw):
    """vehicle_shares + share_paths on a PolygonPlan (plan_polygon_fields) -> (FleetSplit, SharePaths); kw: vehicle_shares' other arguments"""
    split = vehicle_shares(plan.swaths, plan.route, depot, vehicles, radius, spacing=spacing, reversing=reversing, clear_of=clear_of, device=device, **kw)
    return split, share_paths(plan.swaths, split, radius, spacing, reversing=reversing, clear_of=clear_of, device=device)
