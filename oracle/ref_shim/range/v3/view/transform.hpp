// Stand-in for range-v3 0.11.0's views::transform, limited to what the reference headers use: `rng | transform(f)`, a lazy
// view whose begin() and end() may be called on a const view (common/norm.hpp does), each element f(*it) by value.
#pragma once
#include <cstddef>
#include <iterator>
#include <type_traits>
#include <utility>

namespace ranges {
namespace views {

template <class R, class F>
struct transform_view
{
    R r;
    F f;
    using base_iterator = decltype(std::begin(std::declval<R const&>()));

    struct iterator
    {
        base_iterator it;
        F const* f;
        using value_type        = std::decay_t<decltype((*f)(*it))>;
        using reference         = value_type;
        using pointer           = void;
        using difference_type   = std::ptrdiff_t;
        using iterator_category = std::input_iterator_tag;

        reference operator*() const { return (*f)(*it); }
        iterator& operator++()
        {
            ++it;
            return *this;
        }
        iterator operator++(int)
        {
            iterator t = *this;
            ++*this;
            return t;
        }
        bool operator==(iterator const& o) const { return it == o.it; }
        bool operator!=(iterator const& o) const { return it != o.it; }
    };

    iterator begin() const { return {std::begin(r), &f}; }
    iterator end() const { return {std::end(r), &f}; }
};

template <class F>
struct transform_fn
{
    F f;
};

template <class F>
transform_fn<F> transform(F f)
{
    return {std::move(f)};
}

// lvalue ranges are held by reference, rvalues by value
template <class R, class F>
transform_view<R, F> operator|(R&& r, transform_fn<F> t)
{
    return {std::forward<R>(r), std::move(t.f)};
}

} // namespace views
} // namespace ranges
