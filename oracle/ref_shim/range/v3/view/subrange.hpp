// Stand-in for range-v3 0.11.0's make_subrange, limited to what the reference headers use: an iterator pair as a range.
#pragma once

namespace ranges {

template <class I>
struct subrange
{
    I b, e;
    I begin() const { return b; }
    I end() const { return e; }
};

template <class I>
subrange<I> make_subrange(I b, I e)
{
    return {b, e};
}

} // namespace ranges
