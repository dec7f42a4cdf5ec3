"""Handing a torch tensor to an apds_dev_* entry that gets a NULL stream. NULL is the calling thread's own stream, created non-blocking: it
does not order itself behind torch's stream, where torch.full / zeros / ones, in-place ops and device-to-device copies are asynchronous
fill kernels. A buffer pre-filled that way and handed over at once can be filled AFTER the library has written it. (`.to(device)` of a
pageable numpy array synchronises: inputs made that way are safe.)"""


def hand_over():
    """Wait until everything queued on torch's current stream is done: call between the last torch write of a buffer and the ABI call."""
    import torch
    torch.cuda.current_stream().synchronize()
