"""What the "validates before it launches" tests of the C ABI share: an entry point is called on fake device addresses, which are never
dereferenced because validation precedes every launch, with one argument of a valid list replaced at a time."""
BAD_ARG, UNSUPPORTED = -1, -3                # LN3D_ERR_BAD_ARG, LN3D_ERR_UNSUPPORTED
BIG = 1 << 31                                # one more than the largest count


def with_args(args, **at):
    """args with args[k] = v for every keyword i<k>=v"""
    a = list(args)
    for i, v in at.items():
        a[int(i[1:])] = v
    return a


def refuses_null_buffers_and_bad_counts(fn, name, args, buffers, counts):
    """every buffer of `buffers` as a null pointer, and every count of `counts` as zero, negative or oversize, is LN3D_ERR_BAD_ARG"""
    for i in buffers:
        assert fn(*with_args(args, **{'i%d' % i: None})) == BAD_ARG, (name, 'null buffer', i)
    for i in counts:
        for bad in (0, -1, BIG, 1 << 40):
            assert fn(*with_args(args, **{'i%d' % i: bad})) == BAD_ARG, (name, 'count', i, bad)
