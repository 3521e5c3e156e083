"""An independent reader for the files the library reads (include/raytrace_hip.h, "FILE INPUT"): Wavefront OBJ / MTL, PPM (P6 / P3) and
BMP, in plain Python and numpy, written from the rules stated there.  read_obj / read_image raise ValueError("malformed") where the
library returns -2 and FileNotFoundError where it returns -4.  Everything is compared for equal bytes: there are no tolerances.

Numbers: the test files spell every number as the shortest decimal that round-trips a float32 ('%.9g'), for which np.float32(float(tok))
is the correctly rounded value strtof gives; the hand-written spellings (1e-3, -.5, +2., inf, nan) are exact either way."""
import re
import struct
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

NUMBER = re.compile(rb"[+-]?(?:(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|inf|infinity|nan)\Z", re.I)
INDEX = re.compile(rb"-?[0-9]+\Z")
MAP_CHANNEL = {b"map_Kd": 0, b"map_refl": 1, b"map_d": 2, b"map_bump": 3, b"map_Bump": 3, b"bump": 3, b"map_Ke": 4}
SPACE = b" \t\n\v\f\r"  # C's isspace


class Malformed(ValueError):
    def __init__(self):
        super().__init__("malformed")


@dataclass
class Obj:
    points: np.ndarray                      # [P, 3] float32
    polygons: np.ndarray                    # [N, 4] int32, c == d marks a triangle
    corner_normals: Optional[np.ndarray]    # [N, 4, 3] float32, or None when no face has a vn
    corner_uv: Optional[np.ndarray]         # [N, 4, 2] float32, or None when no face has a vt
    polygon_material: np.ndarray            # [N] int32, -1 before the first usemtl
    materials: List[dict] = field(default_factory=list)  # name, kd, ke, has_ke, dissolve, reflect, has_reflect, maps[5] (bytes paths)


def _lines(data: bytes):
    """Lines end at LF; carriage returns are dropped; a NUL ends the line's text.  A last line needs no newline."""
    parts = data.split(b"\n")
    if parts and parts[-1] == b"":
        parts.pop()
    for line in parts:
        yield line.replace(b"\r", b"").split(b"\0", 1)[0]


def _split(line: bytes):
    """(keyword, rest): the line's first token and what follows it, blanks and tabs being the separators."""
    body = line.lstrip(b" \t")
    m = re.match(rb"[^ \t]+", body)
    if not m:
        return None, b""
    return m.group(0), body[m.end():]


def _number(tok: bytes) -> np.float32:
    if not NUMBER.match(tok):
        raise Malformed()
    with np.errstate(over="ignore"):
        return np.float32(float(tok.decode()))


def _numbers(rest: bytes, need: int, want: int):
    toks = _tokens(rest)[:want]
    if len(toks) < need:
        raise Malformed()
    return [_number(t) for t in toks] + [np.float32(0)] * (want - len(toks))


def _tokens(rest: bytes):
    return [t for t in re.split(rb"[ \t]+", rest) if t]


def _name(rest: bytes) -> bytes:
    name = rest.strip(b" \t")
    if not name:
        raise Malformed()
    return name


def _corner(tok: bytes, counts):
    fields = tok.split(b"/")
    if len(fields) > 3 or fields[0] == b"":
        raise Malformed()
    out = [-1, -1, -1]
    for k, f in enumerate(fields):
        if f == b"":
            continue
        if not INDEX.match(f):
            raise Malformed()
        i = int(f)
        if i == 0 or not -2 ** 31 <= i < 2 ** 31:
            raise Malformed()
        at = i - 1 if i > 0 else counts[k] + i
        if not 0 <= at < counts[k]:
            raise Malformed()
        out[k] = at
    return out


def _resolve(obj_path: str, name: bytes) -> bytes:
    if name.startswith(b"/"):
        return name
    cut = obj_path.rfind("/")
    return (obj_path[:cut + 1].encode() if cut >= 0 else b"") + name


def read_obj(path: str) -> Obj:
    with open(path, "rb") as f:
        data = f.read()
    v, vt, vn = [], [], []
    polygons, normals, uvs, poly_mat = [], [], [], []
    mats, ids, libs = [], {}, []
    any_n = any_uv = False
    current = -1

    def material(name: bytes) -> int:
        if name not in ids:
            ids[name] = len(mats)
            mats.append(dict(name=name[:63], kd=[np.float32(1)] * 3, ke=[np.float32(0)] * 3, has_ke=0, dissolve=np.float32(1),
                             reflect=np.float32(0), has_reflect=0, maps=[b""] * 5))
        return ids[name]

    for line in _lines(data):
        key, rest = _split(line)
        if key is None or key.startswith(b"#"):
            continue
        if key == b"v":
            v.append(_numbers(rest, 3, 3))
        elif key == b"vt":
            vt.append(_numbers(rest, 1, 2))
        elif key == b"vn":
            vn.append(_numbers(rest, 3, 3))
        elif key == b"f":
            cs = [_corner(t, (len(v), len(vt), len(vn))) for t in _tokens(rest)]
            if len(cs) < 3:
                raise Malformed()
            faces = [cs] if len(cs) <= 4 else [[cs[0], cs[k], cs[k + 1]] for k in range(1, len(cs) - 1)]
            for face in faces:
                four = [face[min(k, len(face) - 1)] for k in range(4)]
                polygons.append([c[0] for c in four])
                any_uv = any_uv or any(c[1] >= 0 for c in four)
                any_n = any_n or any(c[2] >= 0 for c in four)
                uvs.append([vt[c[1]] if c[1] >= 0 else [np.float32(0)] * 2 for c in four])
                normals.append([vn[c[2]] if c[2] >= 0 else [np.float32(0)] * 3 for c in four])
                poly_mat.append(current)
        elif key == b"usemtl":
            current = material(_name(rest))
        elif key == b"mtllib":
            libs.append(_name(rest))
    for lib in libs:
        try:
            with open(_resolve(path, lib), "rb") as f:
                text = f.read()
        except OSError:
            continue  # a missing library leaves defaults
        at = None
        for line in _lines(text):
            key, rest = _split(line)
            if key is None or key.startswith(b"#"):
                continue
            if key == b"newmtl":
                at = mats[material(_name(rest))]
            elif at is None:
                continue
            elif key == b"Kd":
                at["kd"] = _numbers(rest, 3, 3)
            elif key == b"Ke":
                at["ke"], at["has_ke"] = _numbers(rest, 3, 3), 1
            elif key == b"d":
                at["dissolve"] = _numbers(rest, 1, 1)[0]
            elif key == b"Tr":
                at["dissolve"] = np.float32(1) - _numbers(rest, 1, 1)[0]
            elif key == b"refl":
                at["reflect"], at["has_reflect"] = _numbers(rest, 1, 1)[0], 1
            elif key in MAP_CHANNEL:
                at["maps"] = list(at["maps"])
                at["maps"][MAP_CHANNEL[key]] = _resolve(path, _name(rest))[:255]
    n = len(polygons)
    return Obj(points=np.asarray(v, np.float32).reshape(-1, 3), polygons=np.asarray(polygons, np.int32).reshape(n, 4),
               corner_normals=np.asarray(normals, np.float32).reshape(n, 4, 3) if any_n else None,
               corner_uv=np.asarray(uvs, np.float32).reshape(n, 4, 2) if any_uv else None,
               polygon_material=np.asarray(poly_mat, np.int32).reshape(n), materials=mats)


def record_bytes(m: dict) -> bytes:
    """One material record as the library lays out rtHipObjMaterial (1384 bytes, no padding)."""
    out = m["name"].ljust(64, b"\0") + np.asarray(m["kd"], np.float32).tobytes() + np.asarray(m["ke"], np.float32).tobytes()
    out += struct.pack("<i", m["has_ke"]) + np.float32(m["dissolve"]).tobytes() + np.float32(m["reflect"]).tobytes()
    out += struct.pack("<i", m["has_reflect"]) + b"".join(p.ljust(256, b"\0") for p in m["maps"])
    assert len(out) == 1384
    return out


def obj_arrays(o: Obj) -> dict:
    """The arrays in the library's own layout (4-float points and normals), as bytes; None where the library returns NULL."""
    def pad(a, width):
        out = np.zeros(a.shape[:-1] + (width,), a.dtype)
        out[..., :a.shape[-1]] = a
        return out.tobytes()
    return dict(points=pad(o.points, 4), polygons=o.polygons.tobytes(),
                normals=None if o.corner_normals is None else pad(o.corner_normals, 4),
                uv=None if o.corner_uv is None else o.corner_uv.tobytes(), material=o.polygon_material.tobytes(),
                records=b"".join(record_bytes(m) for m in o.materials))


def material_dicts(o: Obj) -> list:
    """The material records as the dicts frontend.bake_materials takes, by the rules frontend.read_obj states: colour = map_Kd image or
    Kd; transparency on when d < 1 or map_d is given (1x1 of 1 - d, subtracted in float64); reflection on when refl or map_refl is given; bump from map_bump;
    luminance from map_Ke or Ke.  A value becomes a byte as round(value * 255) clipped to 0..255, worked out in float64."""
    def byte3(values):
        return np.clip(np.round(np.asarray([float(x) for x in values], np.float64) * 255.0), 0, 255).astype(np.uint8).reshape(1, 1, 3)
    out = []
    for m in o.materials:
        maps = [p.decode() for p in m["maps"]]
        d = dict(name=m["name"].decode(), rgb=tuple(float(x) for x in m["kd"]), brightness=1.0)
        d["color"] = read_image(maps[0]) if maps[0] else True
        if maps[1]:
            d["reflection"] = read_image(maps[1])
        elif m["has_reflect"]:
            d["reflection"] = byte3([m["reflect"]] * 3)
        if maps[2]:
            d["transparency"] = read_image(maps[2])
        elif m["dissolve"] < 1:
            d["transparency"] = byte3([1.0 - float(m["dissolve"])] * 3)
        if maps[3]:
            d["bump"] = read_image(maps[3])
        if maps[4]:
            d["luminance"] = read_image(maps[4])
        elif m["has_ke"]:
            d["luminance"] = byte3(m["ke"])
        out.append(d)
    return out


def _ppm(data: bytes) -> np.ndarray:
    at = 2
    if len(data) < 3 or data[2] not in SPACE:
        raise Malformed()

    def number():
        nonlocal at
        while True:
            while at < len(data) and data[at] in SPACE:
                at += 1
            if at < len(data) and data[at] == 0x23:  # '#': a comment runs to the end of its line
                while at < len(data) and data[at] != 0x0A:
                    at += 1
            else:
                break
        start = at
        while at < len(data) and 0x30 <= data[at] <= 0x39:
            at += 1
        if at == start:
            raise Malformed()
        value = int(data[start:at])
        if value > 10 ** 9:
            raise Malformed()
        return value

    w, h, maxval = number(), number(), number()
    if w < 1 or h < 1 or not 1 <= maxval <= 255:
        raise Malformed()
    if data[1] == 0x36:  # P6
        if at >= len(data) or data[at] not in SPACE:
            raise Malformed()
        at += 1
        if len(data) - at < 3 * w * h:
            raise Malformed()
        samples = np.frombuffer(data, np.uint8, 3 * w * h, at).astype(np.int64)
    else:
        if len(data) - at < 6 * w * h - 1:
            raise Malformed()
        samples = np.asarray([number() for _ in range(3 * w * h)], np.int64)
    if (samples > maxval).any():
        raise Malformed()
    return (samples * 255 // maxval).astype(np.uint8).reshape(h, w, 3)


def _bmp(data: bytes) -> np.ndarray:
    if len(data) < 54:
        raise Malformed()
    offset, header, width, height = struct.unpack_from("<IIii", data, 10)
    depth, compression = struct.unpack_from("<HI", data, 28)
    if header < 40 or offset < 14 + header or offset > len(data):
        raise Malformed()
    if width < 1 or height == 0 or height == -2 ** 31 or depth not in (24, 32):
        raise Malformed()
    if not (compression == 0 or (compression == 3 and depth == 32)):
        raise Malformed()
    rows = abs(height)
    stride = (width * (depth // 8) + 3) // 4 * 4
    if offset + stride * rows > len(data):
        raise Malformed()
    raster = np.frombuffer(data, np.uint8, stride * rows, offset).reshape(rows, stride)[:, :width * (depth // 8)]
    bgr = raster.reshape(rows, width, depth // 8)[:, :, :3]
    if height > 0:
        bgr = bgr[::-1]  # bottom row first in the file
    return np.ascontiguousarray(bgr[:, :, ::-1])


def read_image(path: str) -> np.ndarray:
    """[h, w, 3] uint8, top row first."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] in (b"P6", b"P3"):
        return _ppm(data)
    if data[:2] == b"BM":
        return _bmp(data)
    raise Malformed()


def image_bytes(img: np.ndarray) -> bytes:
    """The texels in the library's layout: 4 bytes each, (r, g, b, 0)."""
    out = np.zeros(img.shape[:2] + (4,), np.uint8)
    out[:, :, :3] = img
    return out.tobytes()


def fnv1a(data: bytes) -> int:
    """64-bit FNV-1a, the hash tests/fileio_host.cpp prints for every array."""
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h
