"""Generate relativepose_amd/csrc/mc_table.h: the 256-case triangle table of relpose_tsdf_mesh, from a face rule and
never typed in.  Two cells that share a face see the same corner signs on it and therefore draw the same segments there, so the mesh is
closed by construction (Lorensen's classic table leaves holes between complementary cases).

  corner c (0..7)   offset (c & 1, c >> 1 & 1, c >> 2 & 1) from the cell's lowest voxel
  case              bit c set iff t(corner c) < 0
  edge e = 4a+u+2v  along axis a from the corner whose offsets on the other two axes, ascending, are (u, v); its vertex is the crossing that
                    corner's voxel owns on axis a
  faces             the four corners of each cube face counter-clockwise seen from outside; per maximal run of negative corners on the
                    cycle one directed segment, from the crossing edge that enters the run to the one that leaves it (a face of
                    alternating signs gets two segments, each cutting off one negative corner)
  loops             every crossing edge has one outgoing and one incoming segment: disjoint directed loops, ordered by smallest edge id
  triangles         per loop a fan (q0, qk, qk+1) in loop direction; the apex q0 is the loop vertex with the fewest fan diagonals that join
                    two edges of one cube face, ties to the smallest edge id (no in-face diagonal remains in any case)

    python tools/gen_mc_table.py            writes the header
    python tools/gen_mc_table.py --check    exits 1 if the committed header differs
"""
import os
import sys

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "relativepose_amd", "csrc", "mc_table.h")
MAX_TRIANGLES = 5


def corner_offset(c):
    return (c & 1, c >> 1 & 1, c >> 2 & 1)


def corner_index(p):
    return p[0] + 2 * p[1] + 4 * p[2]


def edge_ends(e):
    """-> (offset of the owning corner, offset of the other end)"""
    a, u, v = e // 4, e % 4 & 1, e % 4 >> 1
    o = [x for x in range(3) if x != a]
    p = [0, 0, 0]
    p[o[0]], p[o[1]] = u, v
    q = list(p)
    q[a] = 1
    return tuple(p), tuple(q)


EDGE_CORNERS = [tuple(corner_index(p) for p in edge_ends(e)) for e in range(12)]


def edge_between(c0, c1):
    return next(e for e, ab in enumerate(EDGE_CORNERS) if set(ab) == {c0, c1})


def face_cycle(f, s):
    """the corners of the face axis f = s, counter-clockwise seen from outside the cube"""
    o = [x for x in range(3) if x != f]
    pts = []
    for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
        p = [0, 0, 0]
        p[f], p[o[0]], p[o[1]] = s, u, v
        pts.append(p)
    d1, d3 = [pts[1][x] - pts[0][x] for x in range(3)], [pts[3][x] - pts[0][x] for x in range(3)]
    n = (d1[1] * d3[2] - d1[2] * d3[1], d1[2] * d3[0] - d1[0] * d3[2], d1[0] * d3[1] - d1[1] * d3[0])
    if n[f] * (1 if s else -1) < 0:
        pts = pts[::-1]
    return [corner_index(p) for p in pts]


FACES = [face_cycle(f, s) for f in range(3) for s in range(2)]
EDGE_FACES = [{fi for fi, cyc in enumerate(FACES) if a in cyc and b in cyc} for a, b in EDGE_CORNERS]


def case_loops(case):
    """-> the directed loops of edge ids, ordered by smallest edge id, each starting at its smallest edge id"""
    neg = [case >> c & 1 for c in range(8)]
    nxt = {}
    for cyc in FACES:
        sg = [neg[c] for c in cyc]
        if sum(sg) in (0, 4):
            continue
        for i in range(4):
            if sg[i] and not sg[i - 1]:
                j = i
                while sg[(j + 1) % 4]:
                    j = (j + 1) % 4
                e_in, e_out = edge_between(cyc[i - 1], cyc[i]), edge_between(cyc[j], cyc[(j + 1) % 4])
                assert e_in not in nxt
                nxt[e_in] = e_out
    assert sorted(nxt) == sorted(nxt.values())
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        lp, x = [e], nxt[e]
        seen.add(e)
        while x != e:
            lp.append(x)
            seen.add(x)
            x = nxt[x]
        loops.append(lp)
    return loops


def in_face_diagonals(q):
    """the fan diagonals (q0, qk) of the loop q that join two edges of one cube face"""
    return sum(1 for k in range(2, len(q) - 1) if EDGE_FACES[q[0]] & EDGE_FACES[q[k]])


def case_triangles(case):
    tris = []
    for lp in case_loops(case):
        q = min((lp[r:] + lp[:r] for r in range(len(lp))), key=lambda q: (in_face_diagonals(q), q[0]))
        tris += [(q[0], q[k], q[k + 1]) for k in range(1, len(q) - 1)]
    return tris


def table():
    """-> [256] lists of (e0, e1, e2) edge-id triangles"""
    return [case_triangles(c) for c in range(256)]


def packed(tris):
    """one case as the header's 64-bit word: the triangle count in bits 60..62, the edge id of corner j of triangle t in bits 4(3t+j)..+3"""
    assert len(tris) <= MAX_TRIANGLES
    w = len(tris) << 60
    for t, tri in enumerate(tris):
        for j, e in enumerate(tri):
            w |= e << 4 * (3 * t + j)
    return w


def header_text():
    T = table()
    lines = ["// Generated by tools/gen_mc_table.py -- do not edit; tests/test_mesh_cpu.py regenerates and compares.",
             "// The marching-cubes case table of relpose_tsdf_mesh (DESIGN.md §4.18): case = the 8-bit mask of negative corners (corner c at offset",
             "// (c & 1, c >> 1 & 1, c >> 2 & 1)); rp_mc_table[case] holds the number of triangles (0..5) in bits 60..62 and the edge id of corner j of",
             "// triangle t in bits 4 (3 t + j) .. 4 (3 t + j) + 3.  Edge 4 a + u + 2 v runs along axis a from the corner whose offsets on the other",
             f"// two axes, ascending, are (u, v).  {sum(len(t) for t in T)} triangles in all.",
             "#pragma once",
             "",
             "static __device__ const unsigned long long rp_mc_table[256] = {"]
    for r in range(0, 256, 4):
        lines.append("    " + " ".join(f"0x{packed(T[c]):016x}ull," for c in range(r, r + 4)))
    lines += ["};", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    text = header_text()
    if "--check" in sys.argv:
        sys.exit(0 if open(HEADER).read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print(HEADER)
