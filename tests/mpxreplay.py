"""The routing loop around a multiplexer object, driven by intermediates known per tuple: what POLARPipelineExecutor does
with PhysicalMultiplexer::Execute, the cache-flushing skips and FinalizePathRun, without any join.  Works on the host
mirror's HostMultiplexer and on the oracle's Multiplexer (both expose execute / add_intermediates / increase_input /
finalize_path_run)."""

ALL_CHUNKS = 2**64 - 1  # cache_skips of a strategy that never asks again (DEFAULT_PATH, INIT_ONCE after its init phase)


def replay(mpx, prefix, n, vector_size=1024, chunk_offsets=None, watch=None):
    """prefix[t, p] = intermediates tuples [0, t) produce on join order p.  Routes the n tuples chunk by chunk and closes the
    last run.  Returns (rounds, slices): rounds = [[path, tuples, intermediates]] per routing round (an Execute and the
    whole chunks that follow it on the same path), slices = [(path, tuples)] per chunk or part of a chunk handed to a path.
    watch(mpx, begin): called after every Execute with the first tuple of its slice."""
    if chunk_offsets is None:
        chunk_offsets = list(range(0, n, vector_size)) + [n]
    n_chunks = len(chunk_offsets) - 1
    rounds, slices = [], []
    c, skips, in_process, cur_path = 0, 0, False, 0
    while c < n_chunks:
        c0, size = int(chunk_offsets[c]), int(chunk_offsets[c + 1] - chunk_offsets[c])
        if skips > 0 and not in_process:
            # the path of a bypass chunk = the current path of the multiplexer
            take = min(skips, n_chunks - c)
            begin, end = c0, int(chunk_offsets[c + take])
            mpx.increase_input(end - begin)
            if skips != ALL_CHUNKS:
                skips -= take
            if hasattr(mpx, "set_skips"):
                mpx.set_skips(skips)
            for x in range(c, c + take):
                slices.append((cur_path, int(chunk_offsets[x + 1] - chunk_offsets[x])))
            c += take
        else:
            more, off, cnt, cur_path, skips = mpx.execute(size)
            begin, end = c0 + off, c0 + off + cnt
            in_process = more
            if not more:
                c += 1
            rounds.append([cur_path, 0, 0])
            slices.append((cur_path, cnt))
            if watch is not None:
                watch(mpx, begin)
        inter = int(prefix[end, cur_path] - prefix[begin, cur_path])
        mpx.add_intermediates(inter)
        rounds[-1][1] += end - begin
        rounds[-1][2] += inter
    mpx.finalize_path_run()
    return rounds, slices
