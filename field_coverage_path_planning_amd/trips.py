"""Service trips: a routed field split into capacity-limited round trips to a service point -- a water tank, a trailer at the gate -- and
every trip driven as a path of its own (fcpp_trip_solve; the rule: include/fcpp.h).  A module of its own beside engine, whose public
surface stays what it is; it uses engine's binding layer and the helpers route_swaths itself prices its connectors with."""
import dataclasses
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from . import engine as E
from .engine import _dev_f64, _host_ptr, _one_per, _owners, _ptr, _torch, get_context


@dataclass
class TripSplit:
    """service_trips(): for every field the tour that is driven and where it is left for the service point.  Field i owns the positions
    offsets_host[i] .. offsets_host[i + 1] of `tour` and `trip` (the SwathSet's offsets) and the trips trip_offsets_host[i] ..
    trip_offsets_host[i + 1]; trip k owns the positions trip_swath_offsets[k] .. trip_swath_offsets[k + 1] of `tour`."""
    offsets_host: object        # (n + 1) int64, numpy
    tour: object                # (m) int32, device: oriented swaths 2 s + d in driving order, as SwathRoute.order holds them
    trip: object                # (m) int32: per tour position the trip's index within the field, from 0, never decreasing
    n_trips: object             # (n) int32
    overfull: object            # (n) int32: the trips of ONE swath that is longer than the capacity: the vehicle refills mid-swath, which is not planned
    winner: object              # (n) int32: the variant 2 c + r that gave `tour`: candidate c, r = 1 driven backwards
    status: object              # (n) int32: 0, FCPP_EUNSUPPORTED (more than 512 swaths) or FCPP_EINVAL: candidate 0 as one trip, NaN costs
    cost: object                # (n) float64: the connectors of all trips plus stop_cost per stop [m]: base + extra
    base: object                # (n) float64: the tour's connectors without a stop, as the router prices them
    extra: object               # (n) float64: what the stops add
    costs: object               # (n, 2 C) float64: every variant's cost, NaN for the backward ones with both_ways=False
    trip_offsets: object        # (n + 1) int64, device; trip_offsets_host: the numpy copy
    trip_offsets_host: object
    trip_swath_offsets: object  # (trips + 1) int64, device: into `tour`
    trip_field: object          # (trips) int64: the field of every trip
    trip_work: object           # (trips) float64: the summed swath length of every trip [m]
    stops: object               # (n) int32: n_trips - 1, 0 for a field without swaths
    service: object             # (n, 3) float64: the service pose of every field
    entry: object = None        # (n, 3) or None: where the first trip starts, if not at the service pose
    exit: object = None         # (n, 3) or None: where the last trip ends
    stop_cost: float = 0.0

    def field(self, i):
        """(tour, trip) of field i"""
        sl = slice(int(self.offsets_host[i]), int(self.offsets_host[i + 1]))
        return self.tour[sl], self.trip[sl]


def _poses(pose, n, dev, name):
    p = _dev_f64(pose, dev).reshape(-1, 3)
    if p.shape[0] != n:
        raise ValueError('%s must hold one pose (x, y, heading) per field' % name)
    return p.contiguous()


def _transit_chunks(ctx, ss, R, reversing, pf, penalty, price_clear):
    """(lo, hi, chunk, T) over the fields of a SwathSet in route_swaths' chunks, every chunk's transit blocks as route_swaths prices them"""
    ro_h = vo_h = None
    if pf is not None:
        ro_h, vo_h = pf.ring_offsets.cpu().numpy(), pf.vert_offsets.cpu().numpy()
    for lo, hi in E._route_chunks(np.asarray(ss.offsets_host, dtype=np.int64), E.ROUTE_T_BUDGET):
        ch = E._RouteChunk.of(ss, lo, hi)
        if price_clear:
            T, _ = E._route_transit_priced(ctx, ch, R, reversing, E._fields_slice(pf, ro_h, vo_h, lo, hi), penalty)
        else:
            T = E._route_transit(ctx, ch, R, reversing)
            if pf is not None:
                E._route_transit_clear(ctx, ch, R, reversing, E._fields_slice(pf, ro_h, vo_h, lo, hi), penalty, T)
        yield lo, hi, ch, T


def service_trips(swathset, route, service, capacity, radius, spacing=None, reversing=False, entry=None, exit=None, first_capacity=None,
                  stop_cost=0.0, candidates='all', both_ways=True, clear_of=None, price_clear=False, blocked_penalty=1.0e6, device=None):
    """Where to leave a routed field for the service point (fcpp_trip_solve; the rule: include/fcpp.h) -> TripSplit.  `route` is the
    SwathRoute of `swathset`; service: one pose (x, y, heading) per field, where the vehicle is refilled or unloaded; capacity: the work one
    trip may hold, in metres of swath (a scalar or one value per field; +inf: one trip), first_capacity: the same for the first trip (a
    tank that starts part full; None: the capacity); stop_cost >= 0 [m]: a price per stop on top of its driving.  After the swath at
    position j - 1 the vehicle may drive to the service pose and from there to the swath at position j; the stops are chosen so that no
    trip works more than its capacity and the added driving is least -- exactly, by a dynamic programme over the tour.  A swath longer than
    the capacity is a trip of its own and counted in `overfull`.  The tour that is cheapest without stops need not be cheapest with them:
    candidates='all' splits every candidate tour the router kept (route.tours), 'route' only route.order; both_ways=True also splits each
    one driven backwards; the cheapest total wins (TripSplit.winner).
    entry / exit (one pose per field): where the first trip starts and the last one ends; None: at the service pose.  Transits and the
    ways to and from the poses are priced as route_swaths prices them -- pass the same radius, spacing, reversing, clear_of, price_clear and
    blocked_penalty -- so a trip's connectors cost what trip_paths drives.  Fields are solved in route_swaths' chunks of at most
    ROUTE_T_BUDGET bytes of transit blocks.  A field of more than 512 swaths, or with a capacity <= 0, is one trip over route's candidate 0
    (status FCPP_EUNSUPPORTED / FCPP_EINVAL)."""
    if candidates not in ('all', 'route'):
        raise ValueError("candidates must be 'all' or 'route'")
    if price_clear and clear_of is None:
        raise ValueError('price_clear=True needs clear_of: the region the connectors have to stay clear of')
    ctx = get_context(device)
    torch = _torch()
    ss = swathset
    dev = ss.a.device
    R = float(radius) if spacing is None else E._chord_radius(radius, spacing)
    soff_all = np.asarray(ss.offsets_host, dtype=np.int64)
    n, m_total = len(soff_all) - 1, int(soff_all[-1])
    srv = _poses(service, n, dev, 'service')
    ent = None if entry is None else _poses(entry, n, dev, 'entry')
    ext = None if exit is None else _poses(exit, n, dev, 'exit')
    Q = _one_per(_dev_f64(capacity, dev), n, 'capacity', 'value per field')
    Q0 = None if first_capacity is None else _one_per(_dev_f64(first_capacity, dev), n, 'first_capacity', 'value per field')
    tours = (route.tours if candidates == 'all' else route.order.reshape(1, -1)).to(torch.int32)
    C = int(tours.shape[0])
    if int(tours.shape[1]) != m_total:
        raise ValueError('route must be the SwathRoute of the SwathSet')
    pf = None if clear_of is None else E._clear_fields(clear_of, n, device)
    ends = lambda pose, at_entry: E._route_ends(ss, pose, at_entry, R, reversing, device, pf, blocked_penalty, price_clear)
    In_all, Out_all = ends(srv, True), ends(srv, False)
    E_all = In_all if ent is None else ends(ent, True)
    X_all = Out_all if ext is None else ends(ext, False)
    tour, trip = (torch.empty(m_total, dtype=torch.int32, device=dev) for _ in range(2))
    n_trips, overfull, winner, status = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    cost, base, extra = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
    costs = torch.empty((n, 2 * C), dtype=torch.float64, device=dev)
    for lo, hi, ch, T in _transit_chunks(ctx, ss, R, reversing, pf, blocked_penalty, price_clear):
        s0, m = int(soff_all[lo]), ch.m
        part = lambda a: a[2 * s0:2 * (s0 + m)]
        tr = tours[:, s0:s0 + m].contiguous()
        ctx.bind_stream()
        L.check(ctx.lib.fcpp_trip_solve(ctx.handle, hi - lo, _ptr(ch.soff), _host_ptr(ch.soff_h), m, _ptr(ch.toff), _host_ptr(ch.toff_h),
                                        int(ch.toff_h[-1]), _ptr(T), _ptr(ss.length[s0:s0 + m]), _ptr(part(E_all)), _ptr(part(X_all)), _ptr(part(In_all)),
                                        _ptr(part(Out_all)), C, _ptr(tr), 1 if both_ways else 0, _ptr(Q[lo:hi]), _ptr(Q0[lo:hi]) if Q0 is not None else _ptr(None),
                                        float(stop_cost), _ptr(tour[s0:s0 + m]), _ptr(trip[s0:s0 + m]), _ptr(n_trips[lo:hi]), _ptr(overfull[lo:hi]),
                                        _ptr(winner[lo:hi]), _ptr(status[lo:hi]), _ptr(cost[lo:hi]), _ptr(base[lo:hi]), _ptr(extra[lo:hi]), _ptr(costs[lo:hi])))
    # the trips as a CSR table over the tour
    nt_h = n_trips.cpu().numpy().astype(np.int64)
    toff_h = np.concatenate([[0], np.cumsum(nt_h)]).astype(np.int64)
    toff = torch.as_tensor(toff_h, device=dev)
    K = int(toff_h[-1])
    field_of = _owners(ss.offsets, m_total)
    global_trip = trip.to(torch.int64) + toff[:-1][field_of]
    per_trip = torch.bincount(global_trip, minlength=K) if m_total else torch.zeros(K, dtype=torch.int64, device=dev)
    tso = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(per_trip, 0)])
    swath = ss.offsets[field_of] + (tour.to(torch.int64) >> 1)
    work = torch.zeros(K, dtype=torch.float64, device=dev).index_add_(0, global_trip, ss.length[swath])
    return TripSplit(soff_all, tour, trip, n_trips, overfull, winner, status, cost, base, extra, costs, toff, toff_h, tso, _owners(toff, K), work,
                     (n_trips - 1).clamp(min=0), srv, ent, ext, float(stop_cost))


@dataclass
class TripPaths(E.FieldPaths):
    """trip_paths(): one sampled path per TRIP: a FieldPaths whose path k is trip k's, over `swaths`, the SwathSet whose "fields" are the
    trips.  Every trip starts and ends at its field's service pose, but the first trip of a field with an entry pose and the last one of
    a field with an exit pose."""
    swaths: object = None       # SwathSet: the swath records regrouped by trip, in driving order
    trip_field: object = None   # (trips) int64: the field of every trip
    trip_first: object = None   # (trips) int64: the trip's first position within its field's tour
    trip_index: object = None   # (trips) int64: the trip's index within its field

    def path_field(self):
        return self.trip_field

    def pass_id(self):
        """the leg's slot as the undivided path of the same tour numbers it, moved on by the trip's index: unique over a field's trips"""
        owner = _owners(self.offsets, int(self.x.numel()))
        return (self.leg.to(_torch().int64) + (2 * self.trip_first + self.trip_index)[owner]).to(_torch().int32)


def _gather_fields(pf, idx_h):
    """the fields idx_h (numpy) of a PolygonFields, in that order, as a PolygonFields of their own"""
    torch = _torch()
    dev = pf.x.device
    ro_h, vo_h = pf.ring_offsets.cpu().numpy(), pf.vert_offsets.cpu().numpy()

    def ranges(first, count):
        """the concatenated ranges first[k] .. first[k] + count[k]"""
        off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
        return np.repeat(first - off[:-1], count) + np.arange(int(off[-1]), dtype=np.int64), off

    rings, ring_off = ranges(ro_h[idx_h], ro_h[idx_h + 1] - ro_h[idx_h])
    verts, vert_off = ranges(vo_h[rings], vo_h[rings + 1] - vo_h[rings])
    v = torch.as_tensor(verts, device=dev)
    return E.PolygonFields(torch.as_tensor(ring_off, device=dev), torch.as_tensor(vert_off, device=dev), pf.x[v].contiguous(), pf.y[v].contiguous())


def _regrouped(swathset, tour, group_swath_offsets, group_field):
    """The swath records of a SwathSet regrouped along each field's `tour` (m_total oriented swaths, field-local) into the groups that own
    the positions group_swath_offsets[k] .. group_swath_offsets[k + 1] of it -> (the SwathSet whose "fields" are the groups, its records in
    driving order; the order that drives each group as the tour does).  group_field: the field of every group.  What trip_paths does for
    the trips and fleet.share_paths for the vehicles' shares."""
    torch = _torch()
    ss = swathset
    dev = ss.a.device
    m_total = int(tour.numel())
    tf = group_field
    field_of = _owners(ss.offsets, m_total)
    tour = tour.to(torch.int64)
    g = ss.offsets[field_of] + (tour >> 1)                    # the swath record driven at every tour position
    tso = group_swath_offsets
    tso_h = tso.cpu().numpy()
    group_of = _owners(tso, m_total)
    groups = E.SwathSet(tso.contiguous(), tso_h, ss.a[g].contiguous(), ss.b[g].contiguous(), ss.line[g].contiguous(), ss.length[g].contiguous(),
                        ss.status[tf].contiguous(), ss.n_lines[tf].contiguous(), ss.angle[tf].contiguous())
    at = torch.arange(m_total, dtype=torch.int64, device=dev)
    order = (2 * (at - tso[group_of]) + (tour & 1)).to(torch.int32)
    return groups, order


def trip_paths(swathset, split, radius, spacing, reversing=False, clear_of=None, device=None):
    """Every trip of a TripSplit as a sampled path (field_paths over the trips) -> TripPaths.  The swath records are regrouped by trip into a
    SwathSet whose "fields" are the trips (TripPaths.swaths), and field_paths drives each one in the tour's order and directions, from the
    service pose -- or the field's entry pose on its first trip -- to the service pose -- or the field's exit pose on its last trip.
    clear_of (one region per field of `swathset`): every trip's connectors drive the shortest word that stays off its field's region
    (field_paths(clear_of=...)).  path_speeds, trajectory, validate and polygon_coverage take the result as they take any path set; the
    vehicle stands at both ends of every trip."""
    torch = _torch()
    ss = swathset
    dev = ss.a.device
    K = int(split.trip_offsets_host[-1])
    tf = split.trip_field
    tso = split.trip_swath_offsets
    trips, order = _regrouped(ss, split.tour, tso, tf)
    index = torch.arange(K, dtype=torch.int64, device=dev) - split.trip_offsets[tf]
    first = tso[:-1] - ss.offsets[tf]
    srv = split.service[tf]
    ent, ext = srv, srv
    if split.entry is not None:
        ent = torch.where((index == 0).unsqueeze(1), split.entry[tf], srv)
    if split.exit is not None:
        ext = torch.where((index == split.n_trips.to(torch.int64)[tf] - 1).unsqueeze(1), split.exit[tf], srv)
    region = None
    if clear_of is not None:
        region = _gather_fields(E._clear_fields(clear_of, len(split.offsets_host) - 1, device), tf.cpu().numpy())
    fp = E.field_paths(trips, radius, spacing, reversing=reversing, order=order, entry=ent, exit=ext, device=device, clear_of=region)
    return TripPaths(**{f.name: getattr(fp, f.name) for f in dataclasses.fields(fp)}, swaths=trips, trip_field=tf, trip_first=first, trip_index=index)


def plan_trips(plan, service, capacity, radius, spacing, reversing=False, clear_of=None, device=None, **kw):
    """service_trips + trip_paths on a PolygonPlan (plan_polygon_fields) -> (TripSplit, TripPaths); kw: service_trips' other arguments"""
    split = service_trips(plan.swaths, plan.route, service, capacity, radius, spacing=spacing, reversing=reversing, clear_of=clear_of, device=device, **kw)
    return split, trip_paths(plan.swaths, split, radius, spacing, reversing=reversing, clear_of=clear_of, device=device)
