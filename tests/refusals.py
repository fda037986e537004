"""What the tests of the C ABI's host-side refusals share: a refused call returns MGPS_ERR_INVALID_ARGUMENT and leaves a text."""


def refused(status, *words):
    """`status` is MGPS_ERR_INVALID_ARGUMENT and the library's last error holds every one of `words`"""
    from geometricmultigridpressuresolver_amd._lib import lib

    msg = lib().mgps_last_error(None).decode()
    assert status == 1 and all(w in msg for w in words), (status, msg)
