"""Files for the readers of rt_fileio.cpp (include/raytrace_hip.h, "FILE INPUT"), generated from seeds into a directory of the caller's:
a valid corpus, a hand-written table of malformed files with the return code each must get, and seeded random mutations of the corpus.
Every number is written as the shortest decimal that round-trips a float32 ('%.9g'), apart from a handful of hand-written spellings."""
import os
import struct

import numpy as np


def num(x) -> str:
    return "%.9g" % np.float32(x)


def nums(values) -> str:
    return " ".join(num(v) for v in values)


# ---- images ---------------------------------------------------------------------------------------------------------------------------

def p6(img: np.ndarray, maxval: int, header: bytes = None, tail: bytes = b"") -> bytes:
    h, w, _ = img.shape
    head = header if header is not None else b"P6\n%d %d\n%d\n" % (w, h, maxval)
    return head + img.astype(np.uint8).tobytes() + tail


def p3(img: np.ndarray, maxval: int, header: bytes = None, sep: bytes = b" ", tail: bytes = b"\n") -> bytes:
    h, w, _ = img.shape
    head = header if header is not None else b"P3\n%d %d\n%d\n" % (w, h, maxval)
    return head + sep.join(b"%d" % v for v in img.reshape(-1)) + tail


def bmp(img: np.ndarray, bits: int = 24, top_down: bool = False, gap: int = 0, header: int = 40, compression: int = 0, seed: int = 0) -> bytes:
    """img [h, w, 3] RGB -> a BMP: `bits` 24 / 32, rows bottom-up unless top_down, `gap` bytes between the headers and the pixels, an info
    header of `header` bytes (40, or 124 for a V5 header).  Padding, the fourth byte of 32-bit texels and the gap hold seeded noise."""
    rng = np.random.default_rng(1000 + seed)
    h, w, _ = img.shape
    bpp = bits // 8
    stride = (w * bpp + 3) // 4 * 4
    rows = np.frombuffer(rng.bytes(stride * h), np.uint8).reshape(h, stride).copy()
    texel = rows[:, :w * bpp].reshape(h, w, bpp)
    texel[:, :, :3] = img[:, :, ::-1]
    rows[:, :w * bpp] = texel.reshape(h, w * bpp)
    if not top_down:
        rows = rows[::-1]
    offset = 14 + header + gap
    info = struct.pack("<IiiHHIIiiII", header, w, -h if top_down else h, 1, bits, compression, stride * h, 2835, 2835, 0, 0)
    info += rng.bytes(header - 40)  # (masks, colour space and the rest of a V4 / V5 header: not read)
    return b"BM" + struct.pack("<IHHI", offset + stride * h, 0, 0, offset) + info + rng.bytes(gap) + rows.tobytes()


def image_corpus(rng) -> dict:
    def img(h, w, maxval=255):
        return rng.integers(0, maxval + 1, (h, w, 3), dtype=np.uint8)
    files = {
        "p6_1x1.ppm": p6(img(1, 1), 255),
        "p6_1x6.ppm": p6(img(6, 1, 15), 15, b"P6 1 6 15 "),
        "p6_6x1.ppm": p6(img(1, 6, 1), 1, b"P6\t6\r\n1\n1\n"),
        "p6_7x5.ppm": p6(img(5, 7), 255, b"P6\n# a comment\n7 5\n255\n"),
        "p6_comments.ppm": p6(img(5, 7, 15), 15, b"P6 # one\n# two\n7# three\n # four\n5\n#five\n15\n"),
        "p6_tail.ppm": p6(img(2, 3), 255, tail=b"\n# trailing bytes \xff\x00 7 7 7"),
        "p6_space_sample.ppm": p6(np.full((1, 2, 3), 32, np.uint8), 255),      # samples that are white-space bytes themselves
        "p3_1x1.ppm": p3(img(1, 1), 255),
        "p3_1x6.ppm": p3(img(6, 1, 15), 15, sep=b"\n"),
        "p3_6x1.ppm": p3(img(1, 6, 1), 1, b"P3 6 1 1 ", sep=b"\t", tail=b""),  # ends with the last digit
        "p3_7x5.ppm": p3(img(5, 7), 255, sep=b"  "),
        "p3_comments.ppm": p3(img(5, 7, 15), 15, b"P3\n#a\n7 #b\n5 #c\n#d\n15#e\n", sep=b" #s\n"),
        "p3_tail.ppm": p3(img(2, 3), 255, tail=b" 300 trailing junk"),
    }
    k = 0
    for bits in (24, 32):
        for w in range(1, 6):
            top = (w + bits // 8) % 2 == 0
            files[f"bmp{bits}_{w}x{6 - w}_{'top' if top else 'bottom'}.bmp"] = bmp(img(6 - w, w), bits, top, seed=k)
            k += 1
    files["bmp24_3x3_bottom2.bmp"] = bmp(img(3, 3), 24, False, seed=20)
    files["bmp32_2x4_top2.bmp"] = bmp(img(4, 2), 32, True, seed=21)
    files["bmp24_gap.bmp"] = bmp(img(3, 5), 24, False, gap=10, seed=22)
    files["bmp32_v5.bmp"] = bmp(img(2, 3), 32, True, header=124, compression=3, seed=23)
    return files


# ---- OBJ / MTL --------------------------------------------------------------------------------------------------------------------------

def random_obj(rng, faces: int, nl: str = "\n", final_newline: bool = True, materials=(), libs=()) -> bytes:
    """A seeded OBJ: triangles, quads, 5- and 9-gons; corners v, v/vt, v//vn, v/vt/vn, v/ and v// mixed over the faces (one form per
    face); positive and negative indices; usemtl lines between the faces."""
    lines = ["# seeded mesh"] + [f"mtllib {lib}" for lib in libs]
    nv = nvt = nvn = 0
    for f in range(faces):
        n = int(rng.choice([3, 3, 4, 4, 5, 9]))
        for _ in range(n):
            lines.append("v " + nums(rng.uniform(-2, 2, 3)))
        nv += n
        form = int(rng.integers(0, 6))
        if form in (1, 3):
            for _ in range(n):
                lines.append("vt " + nums(rng.uniform(0, 1, 2)))
            nvt += n
        if form in (2, 3):
            for _ in range(n):
                lines.append("vn " + nums(rng.normal(size=3)))
            nvn += n
        if materials and f and rng.random() < 0.4:
            lines.append("usemtl " + str(rng.choice(materials)))
        neg = rng.random() < 0.5
        toks = []
        for k in range(n):
            def idx(count):
                return str(k - n) if neg else str(count - n + k + 1)
            v = idx(nv)
            toks.append({0: v, 1: f"{v}/{idx(nvt)}", 2: f"{v}//{idx(nvn)}", 3: f"{v}/{idx(nvt)}/{idx(nvn)}", 4: v + "/", 5: v + "//"}[form])
        lines.append("f " + " ".join(toks))
    text = nl.join(lines) + (nl if final_newline else "")
    return text.encode()


def obj_corpus(rng, root: str) -> dict:
    """root: where the files will stand (an absolute map path points into it)."""
    files = {}
    files["tri.obj"] = b"".join(b"v " + nums(rng.uniform(-1, 1, 3)).encode() + b"\n" for _ in range(7)) + b"f 1 2 3\nf 3 4 5\nf -1 -2 -3\nf 7 1 4\n"
    files["mixed.obj"] = (
        "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 0.5 1\n"
        "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\nvn 0 0 -1\n"
        "f 1 2 3 4\n"                      # before the first usemtl: material -1, no vt, no vn
        "f 1/ 2/ 5/\nf 2// 3// 5//\n"      # empty fields
        "usemtl side\n"
        "f 3/3/1 4/4/1 5/1/2\nf 4/4 1/1 5/2\nf 1//2 2//2 3//2 4//1\n"
        "usemtl top\nf -5/-4/-2 -4/-3/-1 -3/-2/-1 -2/-1/-2\n").encode()
    files["ngon.obj"] = (
        "".join(f"v {num(np.cos(k * 0.7))} {num(np.sin(k * 0.7))} {num(k * 0.125)}\nvt {num(k / 9)} {num(1 - k / 9)}\n" for k in range(9))
        + "usemtl fan\nf 1/1 2/2 3/3 4/4 5/5\nf -9/-9 -8/-8 -7/-7 -6/-6 -5/-5 -4/-4 -3/-3 -2/-2 -1/-1\nf 9 8 7 6 5\n").encode()
    files["layout.obj"] = (
        "# CR LF, tabs, comments, blank lines, extra tokens, no final newline\r\n\r\n"
        "\tv\t0 0 0 1.0\r\n  v  1\t0   0  # w and a remark\r\nv 0 1 0 0.5 0.25 9\r\n   \r\n\t\r\n"
        "o thing\r\ng group one\r\ns off\r\nvp 0.5 0.5\r\nvtx 1 2\r\nvnormal 1 2 3\r\nfoo\r\nl 1 2\r\n"
        "vt 0.25 0.75 0.5\r\nvt\t0.5\r\nvn 0 0 1 extra\r\n"
        "  f 1/1/1\t2/2/1  3/1/1   \r\n#f 1 2 9\r\nf 3 2 1").encode()
    files["spellings.obj"] = (
        "v 1e-3 -.5 +2.\nv 1E2 0.e0 .5e+1\nv inf -inf nan\nv -0 +0 -0.0\nv 3.40282347e+38 1.17549435e-38 16777217\n"
        "vt 1e-3\nvt -.5 +2.\nvn nan inf -inf\nf 1/1/1 2/2/1 3/1/1\nf 4 5 1\n").encode()
    files["blank_names.obj"] = (
        "mtllib lib one.mtl  \t\nmtllib second.mtl\nmtllib missing.mtl\n"
        "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvt 0 0\nvt 1 0\nvt 0 1\n"
        "f 1 2 3\n"
        "usemtl  red brick \t \nf 1/1 2/2 3/3\n"
        "usemtl red brick\nf 2/2 4/1 3/3\n"          # the same material: trailing blanks do not count
        "usemtl never defined\nf 1 2 4\n"
        "usemtl glass\nf 4 2 1\nusemtl   lamp\nf 3 2 1\nusemtl maps\nf 1 3 2\nusemtl more\tmaps\nf 1 4 3\n").encode()
    files["lib one.mtl"] = (
        "# before the first newmtl nothing counts\nKd 0 0 0\nmap_Kd nothing.ppm\n"
        "newmtl red brick  \nKd 0.75 0.25 0.125\nmap_Kd tex one.ppm  \t\n"
        "newmtl defined only\nKd 0.5 0.5 0.5\nKe 1 2 3\n"
        "newmtl glass\n\tKd 0.6 0.7 1 0.5\n\td\t0.4\n  refl 0.3\nTr 0.25\nNs 96\nillum 2\nKdx 9 9 9\n").encode()
    files["second.mtl"] = (
        "newmtl lamp\r\nKe 1 0.9 0.6\r\nd 0.5\r\nTr 0.75\r\nd 0.875\r\n"
        "newmtl maps\r\nmap_Kd a much longer name than the one that replaces it.ppm\r\nmap_Kd p3_7x5.ppm\r\nmap_refl bmp24_3x3_bottom2.bmp\r\nmap_d p6_1x6.ppm\r\nmap_bump bmp32_2x4_top2.bmp\r\nmap_Ke p3_1x1.ppm\r\n"
        f"newmtl more\tmaps\r\nmap_Bump {root}/p6_7x5.ppm\r\nbump p6_1x1.ppm\r\nmap_Bump bmp24_gap.bmp\r\nmap_kd ignored.ppm\r\nmap_Ke {root}/tex one.ppm \r\n"
        "newmtl red brick\r\nrefl 0.0625").encode()
    files["nolib.obj"] = b"v 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl a\nf 1 2 3\nusemtl b\nusemtl c\nf 3 2 1\nusemtl a\nf 2 3 1\n"
    files["empty.obj"] = b""
    files["points_only.obj"] = b"v 1 2 3\nvn 0 1 0\nvt 0.5 0.5\n"
    files["seed_a.obj"] = random_obj(rng, 12)
    files["seed_b.obj"] = random_obj(rng, 12, nl="\r\n", final_newline=False, materials=("m0", "m 1", "glass"), libs=("lib one.mtl",))
    files["seed_c.obj"] = random_obj(rng, 20, materials=("lamp", "maps", "x"), libs=("second.mtl", "lib one.mtl"))
    return files


def write_corpus(root: str, seed: int = 7) -> dict:
    """Writes the valid corpus into root and returns {name: bytes}.  Every map path of its MTL files names an image of the corpus."""
    rng = np.random.default_rng(seed)
    files = image_corpus(rng)
    files["tex one.ppm"] = p6(rng.integers(0, 256, (3, 4, 3), dtype=np.uint8), 255)
    files.update(obj_corpus(rng, root))
    for name, data in files.items():
        with open(os.path.join(root, name), "wb") as f:
            f.write(data)
    return files


# ---- malformed files ----------------------------------------------------------------------------------------------------------------------

TRI = b"v 1 0 0\nv 0 0 1\nv 0 1 0\n"


def _bmp_edit(data: bytes, at: int, fmt: str, value) -> bytes:
    return data[:at] + struct.pack(fmt, value) + data[at + struct.calcsize(fmt):]


def malformed_table() -> list:
    """(label, file name, bytes, expected rc, {other file: bytes}).  One row per rule of "FILE INPUT"; the reproductions of the faults
    the rules were written after stand first."""
    small = np.arange(12, dtype=np.uint8).reshape(2, 2, 3) * 20
    good = bmp(small, 24)
    one = bmp(np.array([[[66, 77, 88]]], np.uint8), 24)
    rows = [
        # the faults found by hand
        ("P6 ends behind maxval, newline form", "a.ppm", b"P6\n1 1\n255", -2, {}),
        ("P6 ends behind maxval, blank form", "a.ppm", b"P6 1 1 255", -2, {}),
        ("bare vt after a longer line", "a.obj", TRI + b"vt\nf 1/1 2/1 3/1\n", -2, {}),
        ("bare vn after a longer line", "a.obj", TRI + b"vn\nf 1//1 2//1 3//1\n", -2, {}),
        ("corner index 4294967297 wraps to 1", "a.obj", TRI + b"f 4294967297 2 3\n", -2, {}),
        ("junk in corner tokens", "a.obj", TRI + b"vt 0 0\nvn 0 0 1\nf 1x 2/1/1/9 3//\n", -2, {}),
        ("P6 sample above maxval", "a.ppm", b"P6 1 1 15\n\xff\x00\x00", -2, {}),
        ("P6 with a letter behind maxval", "a.ppm", b"P6 1 1 255Xabc", -2, {}),
        ("P6 header claiming 30000 x 30000", "a.ppm", b"P6\n30000 30000\n255\n", -2, {}),
        ("P3 header claiming 30000 x 30000", "a.ppm", b"P3\n30000 30000\n255\n", -2, {}),
        ("BMP pixel offset 0", "a.bmp", _bmp_edit(one, 10, "<I", 0), -2, {}),
        # OBJ: keywords and numbers
        ("bare v", "a.obj", TRI + b"v\n", -2, {}),
        ("bare vt with blanks", "a.obj", TRI + b"vt  \t\n", -2, {}),
        ("bare f", "a.obj", TRI + b"f\n", -2, {}),
        ("bare usemtl", "a.obj", TRI + b"usemtl\n", -2, {}),
        ("bare usemtl with blanks", "a.obj", TRI + b"usemtl \t \n", -2, {}),
        ("bare mtllib", "a.obj", TRI + b"mtllib\n", -2, {}),
        ("v with two numbers", "a.obj", b"v 1 2\n", -2, {}),
        ("vn with two numbers", "a.obj", b"vn 1 2\n", -2, {}),
        ("v with a word", "a.obj", b"v 1 2 z\n", -2, {}),
        ("vt with a word", "a.obj", b"vt x\n", -2, {}),
        ("vt whose second token is no number", "a.obj", b"vt 0.5 abc\n", -2, {}),
        ("a number with a tail", "a.obj", b"v 1.5abc 0 0\n", -2, {}),
        ("a lone sign", "a.obj", b"v - 0 0\n", -2, {}),
        ("an exponent without digits", "a.obj", b"v 1e 0 0\n", -2, {}),
        ("a lone point", "a.obj", b"v . 0 0\n", -2, {}),
        ("vtx is no keyword: its face has no vt", "a.obj", TRI + b"vtx 0 0\nf 1/1 2/1 3/1\n", -2, {}),
        ("vnormal is no keyword: its face has no vn", "a.obj", TRI + b"vnormal 0 0 1\nf 1//1 2//1 3//1\n", -2, {}),
        # OBJ: faces
        ("face with two corners", "a.obj", TRI + b"f 1 2\n", -2, {}),
        ("corner 1x", "a.obj", TRI + b"f 1x 2 3\n", -2, {}),
        ("corner with four fields", "a.obj", TRI + b"vt 0 0\nvn 0 0 1\nf 1/1/1/1 2 3\n", -2, {}),
        ("corner with a trailing slash too many", "a.obj", TRI + b"vt 0 0\nvn 0 0 1\nf 1/1/1/ 2 3\n", -2, {}),
        ("corner without v", "a.obj", TRI + b"vt 0 0\nf /1 2 3\n", -2, {}),
        ("corner with a sign only", "a.obj", TRI + b"f - 2 3\n", -2, {}),
        ("corner with a fraction", "a.obj", TRI + b"f 1.0 2 3\n", -2, {}),
        ("index 0", "a.obj", TRI + b"f 0 1 2\n", -2, {}),
        ("vt index 0", "a.obj", TRI + b"vt 0 0\nf 1/0 2/1 3/1\n", -2, {}),
        ("vn index 0", "a.obj", TRI + b"vn 0 0 1\nf 1//0 2//1 3//1\n", -2, {}),
        ("index past the end", "a.obj", TRI + b"f 1 2 4\n", -2, {}),
        ("negative index past the start", "a.obj", TRI + b"f -4 -1 -2\n", -2, {}),
        ("vt index past the end", "a.obj", TRI + b"vt 0 0\nf 1/2 2/1 3/1\n", -2, {}),
        ("vn index past the end", "a.obj", TRI + b"vn 0 0 1\nf 1//1 2//-2 3//1\n", -2, {}),
        ("vt index without any vt", "a.obj", TRI + b"f 1/1 2/1 3/1\n", -2, {}),
        ("vertex defined after its face", "a.obj", b"v 0 0 0\nv 1 0 0\nf 1 2 3\nv 0 1 0\n", -2, {}),
        ("index -4294967297", "a.obj", TRI + b"f -4294967297 2 3\n", -2, {}),
        ("index 4294967295", "a.obj", TRI + b"f 4294967295 2 3\n", -2, {}),
        ("index of 20 digits", "a.obj", TRI + b"f 18446744073709551617 2 3\n", -2, {}),
        ("index 2147483648", "a.obj", TRI + b"f 2147483648 2 3\n", -2, {}),
        # MTL
        ("bare newmtl", "a.obj", TRI + b"mtllib a.mtl\n", -2, {"a.mtl": b"newmtl\n"}),
        ("Kd with two numbers", "a.obj", TRI + b"mtllib a.mtl\n", -2, {"a.mtl": b"newmtl m\nKd 1 2\n"}),
        ("d with a word", "a.obj", TRI + b"mtllib a.mtl\n", -2, {"a.mtl": b"newmtl m\nd opaque\n"}),
        ("bare map_Kd", "a.obj", TRI + b"mtllib a.mtl\n", -2, {"a.mtl": b"newmtl m\nmap_Kd \n"}),
        ("bare Tr after a longer line", "a.obj", TRI + b"mtllib a.mtl\n", -2, {"a.mtl": b"newmtl m\nKd 0.5 0.5 0.5\nTr\n"}),
        # PPM
        ("empty image file", "a.ppm", b"", -2, {}),
        ("one byte", "a.ppm", b"P", -2, {}),
        ("magic only", "a.ppm", b"P6", -2, {}),
        ("P5", "a.ppm", b"P5\n1 1\n255\n\x00\x00\x00", -2, {}),
        ("no white space behind the magic", "a.ppm", b"P61 1 255\nabc", -2, {}),
        ("P6 width 0", "a.ppm", b"P6\n0 1\n255\n\x00\x00\x00", -2, {}),
        ("P6 height 0", "a.ppm", b"P6\n1 0\n255\n\x00\x00\x00", -2, {}),
        ("P6 maxval 0", "a.ppm", b"P6\n1 1\n0\n\x00\x00\x00", -2, {}),
        ("P6 maxval 256", "a.ppm", b"P6\n1 1\n256\n\x00\x00\x00", -2, {}),
        ("P6 maxval 65535", "a.ppm", b"P6\n1 1\n65535\n\x00\x00\x00\x00\x00\x00", -2, {}),
        ("P6 negative width", "a.ppm", b"P6\n-1 1\n255\n\x00\x00\x00", -2, {}),
        ("P6 width of 11 digits", "a.ppm", b"P6\n10000000000 1\n255\n\x00\x00\x00", -2, {}),
        ("P6 one sample short", "a.ppm", b"P6\n2 1\n255\n\x01\x02\x03\x04\x05", -2, {}),
        ("P6 comment behind maxval", "a.ppm", b"P6\n1 1\n255#c\n\x01\x02\x03", -2, {}),
        ("P6 sample above maxval 1", "a.ppm", b"P6 1 1 1 \x01\x00\x02", -2, {}),
        ("P6 1000000000 x 1000000000", "a.ppm", b"P6 1000000000 1000000000 255\n", -2, {}),
        ("P3 sample above maxval", "a.ppm", b"P3\n1 1\n15\n15 16 0\n", -2, {}),
        ("P3 one sample short", "a.ppm", b"P3\n1 1\n255\n1 2\n", -2, {}),
        ("P3 with a word for a sample", "a.ppm", b"P3\n1 1\n255\n1 x 3\n", -2, {}),
        ("P3 negative sample", "a.ppm", b"P3\n1 1\n255\n1 -2 3\n", -2, {}),
        ("P3 maxval 0", "a.ppm", b"P3\n1 1\n0\n0 0 0\n", -2, {}),
        ("P3 ends behind maxval", "a.ppm", b"P3 1 1 255", -2, {}),
        ("P3 1000000000 x 1000000000", "a.ppm", b"P3 1000000000 1000000000 255\n1 2 3", -2, {}),
        # BMP
        ("BMP cut inside the headers", "a.bmp", good[:53], -2, {}),
        ("BMP magic only", "a.bmp", b"BM", -2, {}),
        ("BMP core header of 12 bytes", "a.bmp", _bmp_edit(good, 14, "<I", 12), -2, {}),
        ("BMP header size 39", "a.bmp", _bmp_edit(good, 14, "<I", 39), -2, {}),
        ("BMP pixel offset 53", "a.bmp", _bmp_edit(good, 10, "<I", 53), -2, {}),
        ("BMP pixel offset below a 124-byte header", "a.bmp", _bmp_edit(bmp(small, 32, header=124), 10, "<I", 54), -2, {}),
        ("BMP pixel offset past the end", "a.bmp", _bmp_edit(good, 10, "<I", len(good) + 1), -2, {}),
        ("BMP pixel offset 0xffffffff", "a.bmp", _bmp_edit(good, 10, "<I", 0xFFFFFFFF), -2, {}),
        ("BMP header size 0xfffffff0", "a.bmp", _bmp_edit(good, 14, "<I", 0xFFFFFFF0), -2, {}),
        ("BMP one byte short", "a.bmp", good[:-1], -2, {}),
        ("BMP pixel offset one too far for the rows", "a.bmp", _bmp_edit(good, 10, "<I", 55), -2, {}),
        ("BMP width 0", "a.bmp", _bmp_edit(good, 18, "<i", 0), -2, {}),
        ("BMP width -2", "a.bmp", _bmp_edit(good, 18, "<i", -2), -2, {}),
        ("BMP width 0x7fffffff", "a.bmp", _bmp_edit(good, 18, "<i", 0x7FFFFFFF), -2, {}),
        ("BMP height 0", "a.bmp", _bmp_edit(good, 22, "<i", 0), -2, {}),
        ("BMP height INT32_MIN", "a.bmp", _bmp_edit(good, 22, "<i", -2 ** 31), -2, {}),
        ("BMP height 0x7fffffff", "a.bmp", _bmp_edit(good, 22, "<i", 0x7FFFFFFF), -2, {}),
        ("BMP 30000 x 30000", "a.bmp", _bmp_edit(_bmp_edit(good, 18, "<i", 30000), 22, "<i", 30000), -2, {}),
        ("BMP depth 8", "a.bmp", _bmp_edit(good, 28, "<H", 8), -2, {}),
        ("BMP depth 16", "a.bmp", _bmp_edit(good, 28, "<H", 16), -2, {}),
        ("BMP depth 0", "a.bmp", _bmp_edit(good, 28, "<H", 0), -2, {}),
        ("BMP compression 1", "a.bmp", _bmp_edit(good, 30, "<I", 1), -2, {}),
        ("BMP compression 3 at 24 bits", "a.bmp", _bmp_edit(good, 30, "<I", 3), -2, {}),
        ("BMP compression 4 at 32 bits", "a.bmp", _bmp_edit(bmp(small, 32), 30, "<I", 4), -2, {}),
        ("neither PPM nor BMP", "a.bmp", b"GIF89a" + bytes(60), -2, {}),
    ]
    return rows


PREFIX_P6 = p6(np.arange(18, dtype=np.uint8).reshape(2, 3, 3) + 40, 255, b"P6\n# c\n3 2\n255\n")
PREFIX_P3 = p3(np.arange(12, dtype=np.uint8)[::-1].reshape(2, 2, 3) * 3 + 7, 255, b"P3\n2 2 # c\n255\n", tail=b"\n")
PREFIX_BMP = bmp(np.arange(18, dtype=np.uint8).reshape(2, 3, 3) + 90, 24, seed=5)
PREFIX_OBJ = (b"# prefixes\nmtllib none.mtl\nv 0 0 0\nv 1.5 0 -2\nv 0 1 0.25\nvt 0.5 1\nvn 0 0 1\nusemtl m\nf 1/1/1 2/1/1 -1/1/1\n"
              b"v 1 1 1\nf 1 2 3 4\nf 4//1 3//1 2//1\n")


def prefix_table() -> list:
    """(label, file name, bytes, expected rc or None) for every prefix of one valid P6, P3, BMP and OBJ file.  An image prefix is
    refused unless it holds all samples; for an OBJ prefix the reference reader says which of 0 / -2 applies (None here)."""
    rows = []
    for k in range(len(PREFIX_P6) + 1):
        rows.append((f"P6 prefix {k}", "a.ppm", PREFIX_P6[:k], 0 if k == len(PREFIX_P6) else -2))
    last = len(PREFIX_P3.rstrip(b"\n"))  # the file ends "... 10 7\n": the samples are all there once the one digit of the last is
    assert PREFIX_P3[last - 2:last] == b" 7"
    for k in range(len(PREFIX_P3) + 1):
        rows.append((f"P3 prefix {k}", "a.ppm", PREFIX_P3[:k], 0 if k >= last else -2))
    for k in range(len(PREFIX_BMP) + 1):
        rows.append((f"BMP prefix {k}", "a.bmp", PREFIX_BMP[:k], 0 if k == len(PREFIX_BMP) else -2))
    for k in range(len(PREFIX_OBJ) + 1):
        rows.append((f"OBJ prefix {k}", "a.obj", PREFIX_OBJ[:k], None))
    return rows


# ---- random mutations ---------------------------------------------------------------------------------------------------------------------

def mutate(rng, data: bytes) -> bytes:
    """One seeded mutation: byte flips, a deletion, an insertion or a block swap."""
    b = bytearray(data)
    kind = int(rng.integers(0, 4))
    if not b:
        kind = 2
    if kind == 0:
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, len(b)))
            b[at] = b[at] ^ (1 << int(rng.integers(0, 8))) if rng.random() < 0.5 else int(rng.integers(0, 256))
    elif kind == 1:
        at = int(rng.integers(0, len(b)))
        del b[at:at + int(rng.integers(1, 9))]
    elif kind == 2:
        at = int(rng.integers(0, len(b) + 1))
        what = [rng.bytes(int(rng.integers(1, 5))), b"/", b" ", b"\n", b"-", b"9999999999", b"0", b"#", b"\xff\xff\xff\x7f", b"\x00\x00\x00\x80"]
        b[at:at] = what[int(rng.integers(0, len(what)))]
    else:
        n = int(rng.integers(1, max(2, len(b) // 4)))
        i, j = sorted(int(v) for v in rng.integers(0, max(1, len(b) - n), 2))
        if i + n <= j:
            b[i:i + n], b[j:j + n] = b[j:j + n], b[i:i + n]
        else:
            b[i:i + n] = b[i:i + n][::-1]
    return bytes(b)


def write_mutations(root: str, corpus: dict, per_file: int = 48, seed: int = 99) -> int:
    """Writes per_file mutations of every corpus file into root (which already holds the corpus, so that what a mutated OBJ or MTL still
    names is there).  A mutated MTL comes with a copy of blank_names.obj that names it.  Returns how many were written."""
    rng = np.random.default_rng(seed)
    count = 0
    for name in sorted(corpus):
        stem, ext = os.path.splitext(name)
        for k in range(per_file):
            out = f"mut_{stem.replace(' ', '_')}_{k:02d}"
            data = mutate(rng, corpus[name])
            if ext == ".mtl":
                with open(os.path.join(root, out + ".mtl"), "wb") as f:
                    f.write(data)
                data = corpus["blank_names.obj"].replace(b"mtllib second.mtl", b"mtllib " + out.encode() + b".mtl")
            with open(os.path.join(root, out + (".obj" if ext == ".mtl" else ext)), "wb") as f:
                f.write(data)
            count += 1
    return count


# ---- scenes for the GPU test --------------------------------------------------------------------------------------------------------------

class _ObjText:
    """OBJ lines with running counts, so that a part can name its corners from either end."""
    def __init__(self):
        self.lines, self.nv, self.nvt, self.nvn = [], 0, 0, 0

    def part(self, points, faces, uv=None, normals=None, negative=False, material=None):
        """points [n, 3]; faces: lists of indices into them; uv [n, 2] / normals [n, 3] per point or None."""
        if material is not None:
            self.lines.append("usemtl " + material)
        n = len(points)
        self.lines += ["v " + nums(p) for p in points]
        if uv is not None:
            self.lines += ["vt " + nums(t) for t in uv]
        if normals is not None:
            self.lines += ["vn " + nums(t) for t in normals]
        self.nv += n
        self.nvt += n if uv is not None else 0
        self.nvn += n if normals is not None else 0
        for face in faces:
            toks = []
            for i in face:
                idx = lambda count: str(i - n) if negative else str(count - n + i + 1)
                tok = idx(self.nv)
                if uv is not None or normals is not None:
                    tok += "/" + (idx(self.nvt) if uv is not None else "")
                if normals is not None:
                    tok += "/" + idx(self.nvn)
                toks.append(tok)
            self.lines.append("f " + " ".join(toks))


def _floor(n=8, size=2.0, tile=2.0):
    g = np.linspace(-size, size, n + 1)
    pts = np.array([[x, 0.0, z] for z in g for x in g])
    faces = [[r * (n + 1) + c, r * (n + 1) + c + 1, (r + 1) * (n + 1) + c + 1, (r + 1) * (n + 1) + c] for r in range(n) for c in range(n)]
    return pts, faces, pts[:, [0, 2]] / size * tile, np.tile([0.0, 1.0, 0.0], (len(pts), 1))


def _sphere(centre, radius, seg=8, rings=6):
    pts, uv = [[0.0, 1.0, 0.0]], [[0.5, 1.0]]
    for r in range(1, rings):
        for s in range(seg):
            t, p = np.pi * r / rings, 2 * np.pi * s / seg
            pts.append([np.sin(t) * np.cos(p), np.cos(t), np.sin(t) * np.sin(p)])
            uv.append([s / seg, 1 - r / rings])
    pts.append([0.0, -1.0, 0.0])
    uv.append([0.5, 0.0])
    ring = lambda r, s: 1 + (r - 1) * seg + s % seg
    faces = [[0, ring(1, s + 1), ring(1, s)] for s in range(seg)]
    faces += [[ring(r, s), ring(r, s + 1), ring(r + 1, s + 1), ring(r + 1, s)] for r in range(1, rings - 1) for s in range(seg)]
    faces += [[len(pts) - 1, ring(rings - 1, s), ring(rings - 1, s + 1)] for s in range(seg)]
    unit = np.array(pts)
    return unit * radius + np.asarray(centre), faces, np.array(uv), unit


def _box(lo, hi):
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    pts = np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]])
    faces = [[0, 1, 2, 3], [5, 4, 7, 6], [4, 0, 3, 7], [1, 5, 6, 2], [3, 2, 6, 7], [4, 5, 1, 0]]
    uv = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [1, 0], [0, 0], [0, 1], [1, 1]], float)
    return pts, faces, uv


def _disc(centre, radius, n=12):
    a = 2 * np.pi * np.arange(n) / n
    pts = np.stack([np.cos(a) * radius, np.sin(a) * radius, np.zeros(n)], 1) + np.asarray(centre)
    return pts, [list(range(n))], np.stack([np.cos(a), np.sin(a)], 1) * 0.5 + 0.5


def _panel(x0, x1, y0, y1, z, n=4):
    gx, gy = np.linspace(x0, x1, n + 1), np.linspace(y0, y1, n + 1)
    pts = np.array([[x, y, z] for y in gy for x in gx])
    faces = [[r * (n + 1) + c, r * (n + 1) + c + 1, (r + 1) * (n + 1) + c + 1, (r + 1) * (n + 1) + c] for r in range(n) for c in range(n)]
    uv = np.array([[(x - x0) / (x1 - x0), (y - y0) / (y1 - y0)] for y in gy for x in gx])
    return pts, faces, uv


GPU_CAMERA = dict(eye=(2.6, 2.2, -3.4), look_at=(0.0, 0.4, 0.0), fov=55.0, light_dir=(0.3, -0.8, 0.5))


def write_gpu_scenes(root: str, seed: int = 5) -> list:
    """Three OBJ + MTL scenes of a few hundred triangles with their textures, written into root -> [(OBJ path, names of the materials
    that have an image)].  Between them: faces without a material, faces with and without vn in one mesh, an n-gon fan, negative
    indices, a P3 colour map with maxval 15, a top-down 32-bit BMP bump map, a 1 x N map_d, map_refl and map_Ke.  No degenerate faces."""
    rng = np.random.default_rng(seed)
    img = lambda h, w, lo=0, hi=256: rng.integers(lo, hi, (h, w, 3), dtype=np.uint8)
    grey = lambda h, w, lo=0, hi=256: np.repeat(rng.integers(lo, hi, (h, w, 1), dtype=np.uint8), 3, 2)
    textures = {
        "floor 15.ppm": p3(img(8, 8, 3, 16), 15, b"P3\n# maxval 15\n8 8\n15\n"),
        "bump top.bmp": bmp(grey(6, 5), 32, top_down=True, seed=31),
        "veil.ppm": p6(np.repeat(np.array([0, 255, 40, 220, 0, 255, 90, 255], np.uint8)[:, None, None], 3, 2), 255),       # 1 x 8
        "mirror.ppm": p6(grey(4, 4, 60, 256), 255),
        "glow.bmp": bmp(img(3, 4, 120, 256), 24, seed=32),
        "tiles.bmp": bmp(img(7, 5, 30, 256), 24, top_down=True, gap=6, seed=33),
    }
    for name, data in textures.items():
        with open(os.path.join(root, name), "wb") as f:
            f.write(data)
    scenes = []

    # 0: a smooth sphere without a material, a P3 floor, a mirror box without vn (negative indices), a glowing n-gon
    t = _ObjText()
    t.lines += ["# scene 0", "mtllib gpu0.mtl"]
    p, f, uv, nrm = _sphere((-0.6, 0.7, 0.2), 0.7)
    t.part(p, f, uv, nrm)
    p, f, uv, nrm = _floor()
    t.part(p, f, uv, nrm, material="floor")
    p, f, uv = _box((0.5, 0.0, -0.9), (1.3, 0.9, -0.1))
    t.part(p, f, uv, None, negative=True, material="mirror")
    p, f, uv = _disc((-0.2, 1.2, 1.6), 0.8)
    t.part(p, f, uv, None, material="lamp")
    mtl = ("newmtl floor\nKd 0.8 0.8 0.7\nmap_Kd floor 15.ppm\nnewmtl mirror\nKd 0.9 0.9 0.9\nmap_refl mirror.ppm\n"
           "newmtl lamp\nKd 0.2 0.2 0.2\nmap_Ke glow.bmp\n")
    scenes.append(("gpu0", "\n".join(t.lines) + "\n", mtl, ["floor", "mirror", "lamp"]))

    # 1: a box without a material and without vn, a bumpy floor, a veil with a 1 x N map_d before a reflecting sphere
    t = _ObjText()
    t.lines += ["mtllib gpu1.mtl"]
    p, f, uv = _box((-1.5, 0.0, 0.3), (-0.7, 1.1, 1.1))
    t.part(p, f, None, None, negative=True)
    p, f, uv, nrm = _floor(tile=3.0)
    t.part(p, f, uv, nrm, material="floor")
    p, f, uv, nrm = _sphere((0.4, 0.6, 0.6), 0.6)
    t.part(p, f, None, nrm, material="ball")
    p, f, uv = _panel(-0.2, 1.4, 0.0, 1.4, -0.6)
    t.part(p, f, uv, None, material="veil")
    p, f, uv = _disc((-0.9, 1.0, 1.9), 0.7, n=9)
    t.part(p, f, None, None, negative=True, material="lamp")
    mtl = ("newmtl floor\nKd 0.7 0.8 0.9\nmap_bump bump top.bmp\nnewmtl ball\nKd 0.9 0.4 0.3\nrefl 0.3\n"
           "newmtl veil\nKd 0.9 0.9 0.5\nmap_d veil.ppm\nnewmtl lamp\nKd 0.1 0.1 0.1\nKe 1 0.9 0.6\n")
    scenes.append(("gpu1", "\r\n".join(t.lines) + "\r\n", mtl, ["floor", "veil"]))

    # 2: an n-gon without a material, every map at once, CR LF, the last line without a newline
    t = _ObjText()
    t.lines += ["mtllib gpu2.mtl"]
    p, f, uv = _disc((0.9, 1.1, 1.2), 0.9, n=11)
    t.part(p, f, uv, None)
    p, f, uv, nrm = _floor(n=7, tile=1.5)
    t.part(p, f, uv, nrm, negative=True, material="floor")
    p, f, uv, nrm = _sphere((-0.9, 0.65, -0.2), 0.65, seg=9, rings=5)
    t.part(p, f, uv, nrm, negative=True, material="ball")
    p, f, uv = _box((0.3, 0.0, -1.0), (1.0, 0.7, -0.3))
    t.part(p, f, uv, None, material="cube")
    mtl = ("newmtl floor\nmap_Kd tiles.bmp\nmap_Bump bump top.bmp\nnewmtl ball\nmap_Kd floor 15.ppm\nmap_d veil.ppm\n"
           "newmtl cube\nKd 0.8 0.8 0.8\nmap_refl mirror.ppm\nmap_Ke glow.bmp\n")
    scenes.append(("gpu2", "\r\n".join(t.lines), mtl, ["floor", "ball", "cube"]))

    out = []
    for stem, obj, mtl, textured in scenes:
        with open(os.path.join(root, stem + ".mtl"), "w", newline="") as f:
            f.write(mtl)
        with open(os.path.join(root, stem + ".obj"), "w", newline="") as f:
            f.write(obj)
        out.append((os.path.join(root, stem + ".obj"), textured))
    return out
