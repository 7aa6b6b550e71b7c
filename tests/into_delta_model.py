"""The oracle of the in-place delta pull tests: plain Python over the hub's term lists, the
revisions' bytes and the destinations' addresses.  It shares nothing with zest_amd.into or
zest_amd.delta and works from the definitions:

binding: a file of the base is its header followed by each recorded tensor at its destination's
address, every other byte a hole.  A chunk inside one segment is resident at the segment's address plus
its offset; a chunk that crosses segments without touching a hole is resident in the seam arena
(address ARENA: equal to no destination address); a chunk that touches a hole is not resident.  A
chunk referenced twice keeps its first reference.

pull: a term of the new revision is resident iff every chunk of it is; the others are fetched.  A
resident chunk that overlaps a wanted tensor is kept iff it lies wholly inside the tensor's file
range and its address is dst + (chunk offset - tensor offset); otherwise it is moved.  A term counts as
kept iff it is resident and has a kept chunk.  applied bytes are the overlaps of the wanted
tensors with fetched and with moved chunks."""
from __future__ import annotations

import into_delta_repo as R

ARENA, HEADER = "arena", "header"


def file_chunks(hub, repo: str, path: str):
    """[(xorb index, chunk index, file offset, bytes)] of a file in file order, and its terms as
    [(first, last + 1)] positions in that list."""
    f = hub.repos[("model", repo)].files[path]
    out, terms, off = [], [], 0
    for x, c0, c1 in f.terms:
        cum = hub.xorbs[x].cum
        terms.append((len(out), len(out) + c1 - c0))
        for c in range(c0, c1):
            n = cum[c + 1] - cum[c]
            out.append((x, c, off, n))
            off += n
    assert off == len(f.data), path
    return out, terms


def xet_paths(hub, repo: str):
    return [p for p, f in hub.repos[("model", repo)].files.items() if f.xet_hash]


def layout(data: bytes, addr_of: dict):
    """The segments of a base file over destinations: [(start, end, HEADER | address | None)] covering
    the file; addr_of: {tensor name: address} of the recorded tensors (others are holes)."""
    start, tensors = R.header(data)
    segs, pos = [(0, start, HEADER)], start
    for name, (_, _, off, n) in sorted(tensors.items(), key=lambda kv: (kv[1][2], kv[1][3])):
        if n == 0:
            continue
        if off > pos:
            segs.append((pos, off, None))
        segs.append((off, off + n, addr_of.get(name)))
        pos = off + n
    if pos < len(data):
        segs.append((pos, len(data), None))
    return segs


def place(segs, off: int, n: int):
    """Where the chunk [off, off + n) of a file with these segments is: None (touches a hole),
    (HEADER, offset), an address, or ARENA."""
    touched = [s for s in segs if s[0] < off + n and off < s[1]]
    if any(s[2] is None for s in touched):
        return None
    if len(touched) > 1:
        return ARENA
    s0, _, where = touched[0]
    return (HEADER, off - s0) if where == HEADER else where + (off - s0)


def bind(hub, repo: str, files: dict, addr_of: dict, whole: dict | None = None):
    """{(xorb, chunk): place} of the resident chunks of a base, and (seam chunks, seam bytes,
    boundaries).  files: the base revision's bytes; addr_of: {tensor name: destination address} of what was
    recorded; whole: {path: address of a buffer holding the whole file} for a base that is a Weights."""
    resident, seam_chunks, seam_bytes, boundaries = {}, 0, 0, 0
    for path in xet_paths(hub, repo):
        if path not in files:
            continue
        data = files[path]
        segs = [(0, len(data), whole[path])] if whole is not None else layout(data, addr_of)
        if whole is None and not any(s[2] not in (None, HEADER) for s in segs):
            continue  # nothing of this file was scattered: it is not in the record
        boundaries += len(segs) - 1
        for x, c, off, n in file_chunks(hub, repo, path)[0]:
            at = place(segs, off, n)
            if at is None:
                continue
            if at == ARENA:
                seam_chunks, seam_bytes = seam_chunks + 1, seam_bytes + n
            resident.setdefault((x, c), at)
    return resident, (seam_chunks, seam_bytes, boundaries)


def expect(hub, repo: str, files: dict, resident: dict, dst_of: dict) -> dict:
    """The counters of pull(repo, into=dests, base=...) and per path the same; files: the new
    revision's bytes; dst_of: {wanted tensor name: destination address}."""
    keys = ("kept_terms", "kept_bytes", "moved_chunks", "moved_bytes", "fetched_terms", "fetched_bytes",
            "applied_bytes")
    total, per = dict.fromkeys(keys, 0), {}
    for path in xet_paths(hub, repo):
        _, tensors = R.header(files[path])
        wanted = [(off, n, dst_of[name]) for name, (_, _, off, n) in tensors.items() if name in dst_of and n]
        if not any(name in dst_of for name in tensors):
            continue  # (no index file in these repositories: a file is skipped only by include=)
        chunks, terms = file_chunks(hub, repo, path)
        e = dict.fromkeys(keys, 0)
        e["kept_chunks"], e["moved_set"], e["fetched_term_ids"] = set(), set(), []
        for t, (a, b) in enumerate(terms):
            res = all((x, c) in resident for x, c, _, _ in chunks[a:b])
            kept = moved = 0
            for i in range(a, b):
                x, c, off, n = chunks[i]
                for t_off, t_n, dst in wanted:
                    lo, hi = max(off, t_off), min(off + n, t_off + t_n)
                    if lo >= hi:
                        continue
                    if not res:
                        e["applied_bytes"] += hi - lo
                    elif off >= t_off and off + n <= t_off + t_n and resident[(x, c)] == dst + (off - t_off):
                        kept += 1
                        e["kept_bytes"] += n
                        e["kept_chunks"].add(i)
                    else:
                        e["applied_bytes"] += hi - lo
                        if i not in e["moved_set"]:
                            e["moved_set"].add(i)
                            moved += 1
                            e["moved_bytes"] += n
            if res:
                e["kept_terms"] += int(kept > 0)
                e["moved_chunks"] += moved
            else:
                e["fetched_terms"] += 1
                e["fetched_bytes"] += sum(n for _, _, _, n in chunks[a:b])
                e["fetched_term_ids"].append(t)
        e["chunks"], e["terms"] = chunks, terms
        per[path] = e
        for k in keys:
            total[k] += e[k]
    total["files"] = per
    return total
