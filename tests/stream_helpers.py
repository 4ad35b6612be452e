"""What the GPU tests of the stream pipeline share: the pair-at-a-time sequence the oracle tests pin, and a stream of frames through a
session with the flow of every pair taken while it is among the newest."""


def plain_sequence(eng, frames, w, h, L, win, mode="lk_float", iters=1):
    """flows of every pair of `frames` through the plain pair-at-a-time session (the sequence the oracle tests pin)"""
    import torch

    plain = eng.Session(w, h, L, win, mode, iters=iters)
    plain.set_frame_device(frames[0]); plain.build_pyramid(); plain.swap()
    want = {}
    for i in range(1, len(frames)):
        plain.set_frame_device(frames[i]); plain.build_pyramid(); plain.run_flow()
        torch.cuda.synchronize()
        want[i] = [plain.flow_host(k) for k in range(L)]
        plain.swap()
    plain.close()
    return want


def stream_all_pairs(s, frames, L, B, ptrs=None):
    """every pair of `frames` through the stream pipeline of session s; returns {pair: [flow per level]} (host copies).  ptrs (a dict):
    receives {(pair, level): device address of that flow}"""
    import torch

    got, seen = {}, 0

    def snap(done):
        nonlocal seen
        if done >= 1:
            for p in range(max(seen + 1, done - B + 1), done + 1):
                views = [s.flow_of(p, k)[0] for k in range(L)]
                got[p] = [v.cpu().numpy() for v in views]
                if ptrs is not None:
                    ptrs.update({(p, k): v.data_ptr() for k, v in enumerate(views)})
            seen = done

    s.stream_begin()
    for f in frames:
        snap(s.stream_submit(f))
    while True:
        done = s.stream_drain()
        if done == -2:
            break
        snap(done)
    torch.cuda.synchronize()
    return got
