"""From the shoreline shapefile to the records of the burn and reach entries: the host half of the reference's
_create_ocean_mask (dswx_hls.py:3464-3572), step by step -- select the polygons that meet the tile grown by 2 * margin, clip
them to that box, transform the vertices to the tile SRS; the device then burns them and grows them by the margin
(dswx_burn_device, dswx_reach_device) where the reference calls Buffer(margin_m) and gdal.RasterizeLayer.

No package that reads shapefiles is needed: `read_shp` maps the .shp and reads the record index of the .shx when there is one.
Polygon, PolygonZ and PolygonM records (shape types 5, 15, 25) are read, x and y only; every other type is skipped, as the
reference skips everything that is not 'POLYGON'.  A ring is an OUTER ring when it runs clockwise (negative shoelace area), a
hole otherwise.  OGR reports a record with more than one outer ring as MULTIPOLYGON, which the reference skips: so does `plan`,
and logs how many.

The SRS comes from the .prj: geographic WGS 84 (what GSHHS ships), a WGS 84 / UTM zone, or the SRS of the product itself (equal
EPSG codes).  Everything else is refused, with a message that says what is taken: a missing .prj, a tile box that crosses the
antimeridian (_get_tile_srs_bbox handles it; this does not), product pixels that are not square.

UNPINNED: GDAL, GEOS and PROJ are not available to this project.  Not pinned by execution: GEOS's Intersection against the
Sutherland-Hodgman clip used here (they differ only ON the sides of the clip rectangle, 2 * margin from the tile, where
Sutherland-Hodgman leaves bridging edges between the lobes of a clipped polygon -- the reach table drops every edge that lies on
a side, so that they reach nothing, and the even-odd burn cancels the area between a bridge and the side); OGR's assembly of
rings into polygons (here: orientation alone); PROJ against proteus_amd.warp.tm_forward / tm_inverse (Karney's series, which
PROJ uses too); and the chords of Buffer (inside the circle by at most 3.4e-4 of the margin, include/dswx_hip.h "reach").
"""
import logging
import mmap
import os
import re
import struct

import numpy as np

from . import burn as _burn
from . import reach as _reach
from . import warp

logger = logging.getLogger('dswx_hls')

POLYGON_TYPES = (5, 15, 25)
TAKEN = ('geographic WGS 84 (EPSG:4326, as GSHHS ships), a WGS 84 / UTM zone (EPSG 326zz / 327zz) or the SRS of the product '
         'itself (the same EPSG code in the .prj)')
DROPPED = 0xFFFFFFFF                              # the `next` of a record whose edge takes no part in the reach: malformed


class Shapefile:
    """The polygon records of a .shp: `bbox` float64 [n, 4] (xmin, ymin, xmax, ymax) and `record` int64 [n] (the record's
    position in the file, from 0) of the records of a polygon type, read without touching the points; `rings(i)` reads those of
    polygon i.  `skipped_types` counts the records of every other shape type; `epsg` is what the .prj says (None: no .prj)."""

    def __init__(self, path):
        self.path = os.fspath(path)
        self._file = open(self.path, 'rb')
        self._map = mmap.mmap(self._file.fileno(), 0, access=mmap.ACCESS_READ)
        m = self._map
        if len(m) < 100 or struct.unpack('>i', m[0:4])[0] != 9994 or struct.unpack('<i', m[28:32])[0] != 1000:
            raise ValueError(f'{self.path} is not a shapefile (file code 9994, version 1000)')
        offsets = self._index()
        types = np.array([struct.unpack('<i', m[o + 8:o + 12])[0] if o + 12 <= len(m) else 0 for o in offsets], dtype=np.int64)
        poly = np.isin(types, POLYGON_TYPES)
        self.skipped_types = int((~poly).sum())
        self.record = np.flatnonzero(poly)
        self._offset = np.asarray(offsets, dtype=np.int64)[poly]
        self.bbox = np.array([struct.unpack('<4d', m[o + 12:o + 44]) for o in self._offset], dtype=np.float64).reshape(-1, 4)
        prj = os.path.splitext(self.path)[0] + '.prj'
        self.wkt = open(prj).read() if os.path.exists(prj) else None
        self.epsg = epsg_of_wkt(self.wkt) if self.wkt is not None else None

    def _index(self):
        """The byte offsets of the record headers: from the .shx when there is one, else by walking the .shp."""
        m = self._map
        shx = os.path.splitext(self.path)[0] + '.shx'
        if os.path.exists(shx):
            with open(shx, 'rb') as f:
                raw = f.read()
            n = (len(raw) - 100) // 8
            return (2 * np.frombuffer(raw, dtype='>i4', count=2 * n, offset=100).reshape(n, 2)[:, 0].astype(np.int64)).tolist()
        offsets, at = [], 100
        while at + 8 <= len(m):
            offsets.append(at)
            at += 8 + 2 * struct.unpack('>i', m[at + 4:at + 8])[0]
        return offsets

    def __len__(self):
        return len(self.record)

    def rings(self, i):
        """The rings of polygon i: a list of float64 [k, 2] arrays (x, y) without the repeated closing point, in file order."""
        m, o = self._map, int(self._offset[i]) + 8
        n_parts, n_points = struct.unpack('<2i', m[o + 36:o + 44])
        parts = np.frombuffer(m, dtype='<i4', count=n_parts, offset=o + 44).astype(np.int64)
        pts = np.frombuffer(m, dtype='<f8', count=2 * n_points, offset=o + 44 + 4 * n_parts).reshape(n_points, 2)
        out = []
        for a, b in zip(parts, np.append(parts[1:], n_points)):
            r = np.array(pts[a:b])
            if len(r) > 1 and (r[0] == r[-1]).all():
                r = r[:-1]
            out.append(r)
        return out

    def close(self):
        self._map.close()
        self._file.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_shp(path):
    return Shapefile(path)


def shoelace(ring):
    """Twice the signed area of a ring: negative when it runs clockwise with y up, as an outer ring of a shapefile does."""
    x, y = ring[:, 0], ring[:, 1]
    return float(np.dot(x, np.roll(y, -1)) - np.dot(np.roll(x, -1), y))


def outer_rings(rings):
    """How many of the rings are outer rings (clockwise); a record whose rings all run the other way has one: its first."""
    return max(sum(shoelace(r) < 0 for r in rings), 1 if rings else 0)


def epsg_of_wkt(wkt):
    """4326 for geographic WGS 84, 326zz / 327zz for WGS 84 / UTM, else the EPSG code of the root AUTHORITY when there is
    one, else None.  ESRI's and OGC's spellings."""
    text = wkt.strip()
    wgs84 = re.search(r'WGS[_ ]?(19)?84', text, re.I) is not None
    if re.match(r'GEOGCS|GEOGCRS|GEODCRS', text, re.I):
        return 4326 if wgs84 else _root_authority(text)
    if re.match(r'PROJCS|PROJCRS', text, re.I):
        zone = re.search(r'UTM[_ ]zone[_ ](\d{1,2})\s*([NS])', text, re.I)
        if zone and wgs84 and 1 <= int(zone.group(1)) <= 60:
            return (32600 if zone.group(2).upper() == 'N' else 32700) + int(zone.group(1))
        return _root_authority(text)
    return None


def _root_authority(text):
    found = re.search(r'(AUTHORITY|ID)\s*\[\s*"EPSG"\s*,\s*"?(\d+)"?\s*\]\s*\]\s*$', text, re.I)
    return int(found.group(2)) if found else None


def clip_side(p, axis, value, keep_above):
    """One side of Sutherland-Hodgman on the open ring p [k, 2], in doubles, all edges at once: an edge p -> q gives the crossing
    when exactly one end is inside, then q when q is.  A crossing has its `axis` coordinate equal to `value` exactly."""
    if len(p) == 0:
        return p
    q, p = p, np.roll(p, 1, axis=0)                          # the edge p -> q that ENDS in vertex i: the order of the textbooks
    pin = p[:, axis] >= value if keep_above else p[:, axis] <= value
    qin = q[:, axis] >= value if keep_above else q[:, axis] <= value
    cross = pin != qin
    span = np.where(cross, q[:, axis] - p[:, axis], 1.0)
    hit = p + ((value - p[:, axis]) / span)[:, None] * (q - p)
    hit[:, axis] = value
    out = np.stack([hit, q], axis=1)
    return out[np.stack([cross, qin], axis=1)]


def clip_ring(ring, rect):
    """The open ring clipped to rect = (xmin, ymin, xmax, ymax), and for every edge of the result (vertex i -> i + 1, cyclic)
    whether it lies ON a side of the rectangle."""
    xmin, ymin, xmax, ymax = rect
    p = np.asarray(ring, dtype=np.float64)
    for axis, value, above in ((0, xmin, True), (0, xmax, False), (1, ymin, True), (1, ymax, False)):
        p = clip_side(p, axis, value, above)
    if len(p):                                               # (a vertex that two sides repeat is kept once)
        p = p[np.append((p[1:] != p[:-1]).any(axis=1), True)]
        if len(p) > 1 and (p[0] == p[-1]).all():
            p = p[:-1]
    q = np.roll(p, -1, axis=0)
    on_side = np.zeros(len(p), dtype=bool)
    for axis, value in ((0, xmin), (0, xmax), (1, ymin), (1, ymax)):
        on_side |= (p[:, axis] == value) & (q[:, axis] == value)
    return p, on_side


class Plan:
    """What `plan` returns: `burn_calls`, a list of (verts, tile_first) tables of ONE tile, each with at most 32 colours (one
    bit of `word` per colour; polygons whose pixel bounding boxes are disjoint share one), to be burnt in place one after the
    other; `reach`, the (verts, tile_first) table of the same edges without those on a side of the clip rectangle; `radius` in
    1/256 pixel; and the counts `polygons`, `colours`, `multipolygons_skipped`, `other_types_skipped`."""

    def __init__(self, burn_calls, reach, radius, counts, rect):
        self.burn_calls, self.reach, self.radius, self.rect = burn_calls, reach, radius, rect
        self.__dict__.update(counts)

    def host_mask(self, height, width, entries=None):
        """The ocean mask uint8 [height, width] (1 = within the margin of land, 0 = ocean) by proteus_amd.burn.burn_tiles and
        proteus_amd.reach.reach_tiles, the numpy statements (`entries`: (burn, reach) callables of the same signature, such as
        _capi.burn_host and _capi.reach_host)."""
        burn, reach = entries or (_burn.burn_tiles, _reach.reach_tiles)
        mask = np.zeros((1, height, width), dtype=np.uint8)
        for verts, first in self.burn_calls:
            mask = np.ascontiguousarray(burn(verts, first, height, width, _burn.Spec(burn=1), src=mask)['mask'])
        return reach(self.reach[0], self.reach[1], height, width, _reach.Spec(self.radius, burn=1), src=mask)['mask'][0]


def colours_of(boxes):
    """Greedy colouring of polygons by their pixel bounding boxes int64 [n, 4] (xmin, ymin, xmax, ymax, closed): every polygon
    takes the lowest colour none of whose polygons' boxes meets its own."""
    colour = np.zeros(len(boxes), dtype=np.int64)
    members = []                                             # per colour: the boxes taken so far
    for i, b in enumerate(boxes):
        for c, taken in enumerate(members):
            t = np.asarray(taken)
            if not ((t[:, 0] <= b[2]) & (t[:, 2] >= b[0]) & (t[:, 1] <= b[3]) & (t[:, 3] >= b[1])).any():
                break
        else:
            c = len(members)
            members.append([])
        members[c].append(b)
        colour[i] = c
    return colour


def _to_product(x, y, src_epsg, dst_epsg):
    if src_epsg == dst_epsg:
        return np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if src_epsg == warp.GEOGRAPHIC_EPSG:
        lon0, fn = warp.utm_zone(dst_epsg)
        e, n = warp.tm_forward(x, y, lon0)
        return e + warp.UTM_FALSE_EASTING, n + fn
    return warp.utm_to_utm(x, y, src_epsg, dst_epsg)


def _from_product(x, y, src_epsg, dst_epsg):
    if src_epsg == dst_epsg:
        return np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if src_epsg == warp.GEOGRAPHIC_EPSG:
        lon0, fn = warp.utm_zone(dst_epsg)
        return warp.tm_inverse(np.asarray(x, dtype=np.float64) - warp.UTM_FALSE_EASTING, np.asarray(y, dtype=np.float64) - fn, lon0)
    return warp.utm_to_utm(x, y, dst_epsg, src_epsg)


def plan(shp, geotransform, product_epsg, length, width, margin_m):
    """The tables that turn the shoreline polygons of `shp` (a path or a Shapefile) into the ocean mask of a product of length
    x width pixels with `geotransform` in the SRS `product_epsg`, the land grown by `margin_m` metres: a Plan."""
    own = not isinstance(shp, Shapefile)
    shp = read_shp(shp) if own else shp
    try:
        return _plan(shp, [float(v) for v in geotransform], product_epsg, int(length), int(width), float(margin_m))
    finally:
        if own:
            shp.close()


def srs_of(shp, product_epsg=None):
    """The EPSG code of the shapefile's .prj; refused when there is no .prj, or when the SRS is none that is taken (without
    `product_epsg`: whatever code the .prj names may still be the product's)."""
    if shp.wkt is None:
        raise NotImplementedError(f'shoreline_shapefile: {shp.path} has no .prj beside it; the SRS of a shoreline must be {TAKEN}')
    src = shp.epsg
    utm = src is not None and src // 100 in (326, 327) and 1 <= src % 100 <= 60
    if src is None or not (src == warp.GEOGRAPHIC_EPSG or utm or product_epsg is None or src == product_epsg):
        raise NotImplementedError(f'shoreline_shapefile: the SRS of {shp.path} (EPSG {src}) is not taken; the SRS of a shoreline must be '
                                  f'{TAKEN}')
    return src


def _plan(shp, gt, product_epsg, length, width, margin_m):
    src = srs_of(shp, product_epsg if product_epsg is not None else 0)
    if src != product_epsg:
        try:
            warp.utm_zone(product_epsg)
        except ValueError as e:
            raise NotImplementedError(f'shoreline_shapefile: the product is not in a WGS 84 / UTM zone ({e}); the SRS of a shoreline '
                                      f'must then be that of the product. Taken: {TAKEN}')
    if gt[2] != 0.0 or gt[4] != 0.0 or abs(gt[1]) != abs(gt[5]) or gt[1] <= 0.0 or gt[5] >= 0.0:
        raise NotImplementedError(f'shoreline_shapefile: product pixels of {gt[1]} x {gt[5]} (rotation {gt[2]}, {gt[4]}) are not square '
                                  'and north-up: the margin is one radius in pixels')
    pixel = gt[1]
    radius = int(round(256.0 * margin_m / pixel))
    if not 0 <= radius <= _reach.MAX_RADIUS:
        raise NotImplementedError(f'shoreline_shapefile: a margin of {margin_m} m is {radius / 256:.1f} pixels of {pixel} m, above the '
                                  f'{_reach.MAX_RADIUS // 256} pixels of the reach entries')
    # the tile grown by 2 * margin, its four corners in the SRS of the polygons, their min / max rectangle (:3434-3457)
    x0, x1 = gt[0] - 2 * margin_m, gt[0] + width * gt[1] + 2 * margin_m
    y1, y0 = gt[3] + 2 * margin_m, gt[3] + length * gt[5] - 2 * margin_m
    cx, cy = _from_product(np.array([x0, x1, x1, x0]), np.array([y1, y1, y0, y0]), src, product_epsg)
    rect = (float(cx.min()), float(cy.min()), float(cx.max()), float(cy.max()))
    if src == warp.GEOGRAPHIC_EPSG and (rect[2] > rect[0] + 340 or rect[0] < -180.0 or rect[2] > 180.0):
        raise NotImplementedError(f'shoreline_shapefile: the tile reaches {rect[0]:.4f} .. {rect[2]:.4f} degrees of longitude: the '
                                  'antimeridian is not handled')
    b = shp.bbox
    chosen = np.flatnonzero((b[:, 0] <= rect[2]) & (b[:, 2] >= rect[0]) & (b[:, 1] <= rect[3]) & (b[:, 3] >= rect[1])) if len(b) else []
    polygons, multi = [], 0                                  # per polygon: [(ring int32 [k, 2], on_side bool [k])]
    for i in chosen:
        rings = shp.rings(int(i))
        if outer_rings(rings) > 1:
            multi += 1
            continue
        mine = []
        for ring in rings:
            p, on_side = clip_ring(ring, rect)
            if len(p) < 3:
                continue
            x, y = _to_product(p[:, 0], p[:, 1], src, product_epsg)
            mine.append((_burn.quantise(np.stack([(x - gt[0]) / gt[1], (y - gt[3]) / gt[5]], axis=1)), on_side))
        if mine:
            polygons.append(mine)
    if multi:
        logger.info(f'    shoreline: {multi} record(s) with more than one outer ring (MULTIPOLYGON) skipped, as the reference does')
    boxes = np.array([[min(r[:, 0].min() for r, _ in m), min(r[:, 1].min() for r, _ in m),
                       max(r[:, 0].max() for r, _ in m), max(r[:, 1].max() for r, _ in m)] for m in polygons], dtype=np.int64).reshape(-1, 4)
    boxes = np.stack([boxes[:, 0] >> 8, boxes[:, 1] >> 8, (boxes[:, 2] >> 8) + 1, (boxes[:, 3] >> 8) + 1], axis=1)
    colour = colours_of(boxes)
    n_colours = int(colour.max()) + 1 if len(colour) else 0
    burn_calls = []
    for c0 in range(0, max(n_colours, 1), 32):
        mine = [j for j in range(len(polygons)) if c0 <= colour[j] < c0 + 32]
        rings = [r for j in mine for r, _ in polygons[j]]
        words = [1 << int(colour[j] - c0) for j in mine for _ in polygons[j]]
        burn_calls.append(_burn.tiles([_burn.records(rings, words)]))
    every = [r for m in polygons for r, _ in m]
    verts = _burn.records(every)
    if len(verts):
        verts['next'][np.concatenate([s for m in polygons for _, s in m])] = DROPPED
    counts = {'polygons': len(polygons), 'colours': n_colours, 'multipolygons_skipped': multi, 'other_types_skipped': shp.skipped_types,
              'edges': int(len(verts)), 'edges_on_clip_sides': int((verts['next'] == DROPPED).sum()) if len(verts) else 0}
    return Plan(burn_calls, _burn.tiles([verts]), radius, counts, rect)
