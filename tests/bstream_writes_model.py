"""The grouping rule of a block stream's writer, restated: which groups and chunks BlockCompressorStream writes for a list of write()
sizes.  This is the rule fourmc_gpu_bstreams_compress plans by (include/fourmc_gpu.h, "Block streams from a job's write() calls");
tests/bstream_model.py is the writer itself, buffer by buffer, and the tests hold the two against each other.

With the codecs' 4 MiB buffers a stream's shape depends on its write sizes alone:
  - at write i with nothing accumulated: a write longer than M is a long group of its own, ceil(w / M) chunks, all of M bytes but the
    last; otherwise the group takes writes i .. j for the largest j whose sum stays <= M and is one chunk;
  - a group whose sum is 0 (zero-length writes in front of a long write, or at the end) is not written;
  - the stream ends with BE32(0) when nothing was written or the last written group was a long one."""


def plan(write_sizes, M):
    """([(rawlen, [chunk sizes])], trailer) for write() calls of these sizes"""
    groups, i, n = [], 0, len(write_sizes)
    while i < n:
        w = write_sizes[i]
        if w > M:
            groups.append((w, [M] * (w // M) + ([w % M] if w % M else [])))
            i += 1
            continue
        total, j = 0, i
        while j < n and total + write_sizes[j] <= M:
            total += write_sizes[j]
            j += 1
        if total:
            groups.append((total, [total]))
        i = j
    trailer = not groups or groups[-1][0] > M
    return groups, trailer


def uniform(src_bytes, write_bytes):
    """the schedule of fourmc_bstream_enc_item with n_writes == 0: every write() write_bytes long, the last one short; 0 = one write"""
    if src_bytes == 0:
        return []
    w = write_bytes or src_bytes
    return [w] * (src_bytes // w) + ([src_bytes % w] if src_bytes % w else [])


def worst_case(write_sizes, M, bound):
    """the exact worst case of the stream's length: 4 per written group, 4 + bound(len) per chunk, 4 for the trailer"""
    groups, trailer = plan(write_sizes, M)
    return sum(4 + sum(4 + bound(c) for c in cs) for _, cs in groups) + (4 if trailer else 0)


def max_chunks(S, M):
    """the most chunks any schedule over S bytes has: a 1-byte group in front of a write of M + 1 bytes is 3 chunks in M + 2 bytes"""
    return 3 * (S // (M + 2)) + min(S % (M + 2), 2)


def max_groups(S, M):
    """the most written groups any schedule over S bytes has: a write of 1 then a write of M is 2 groups in M + 1 bytes"""
    return 2 * (S // (M + 1)) + min(S % (M + 1), 1)


def writes_bound(S, M, zstd):
    """fourmc_gpu_bstream_writes_bound: S, the codec's overhead (its share that grows with the bytes, and its constant per chunk),
    4 per chunk, 4 per group and the trailer"""
    C, G = max_chunks(S, M), max_groups(S, M)
    return S + (S // 256 + 64 * C if zstd else S // 255 + 16 * C) + 4 * C + 4 * G + 4
