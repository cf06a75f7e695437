// Stand-in for range-v3 0.11.0's views::zip, limited to what the reference headers use: two ranges walked in step,
// each element a std::tuple of references, the walk ending at the end of the shorter range (as range-v3's zip does).
#pragma once
#include <cstddef>
#include <iterator>
#include <tuple>
#include <utility>

namespace ranges {
namespace views {

template <class A, class B>
struct zip_view
{
    A a;
    B b;
    using ia_type = decltype(std::begin(std::declval<A const&>()));
    using ib_type = decltype(std::begin(std::declval<B const&>()));

    struct iterator
    {
        ia_type ia;
        ib_type ib;
        using value_type        = std::tuple<decltype(*std::declval<ia_type>()), decltype(*std::declval<ib_type>())>;
        using reference         = value_type;
        using pointer           = void;
        using difference_type   = std::ptrdiff_t;
        using iterator_category = std::input_iterator_tag;

        reference operator*() const { return reference(*ia, *ib); }
        iterator& operator++()
        {
            ++ia;
            ++ib;
            return *this;
        }
        iterator operator++(int)
        {
            iterator t = *this;
            ++*this;
            return t;
        }
        // either side at its end ends the walk: the shorter range bounds it
        bool operator==(iterator const& o) const { return ia == o.ia || ib == o.ib; }
        bool operator!=(iterator const& o) const { return !(*this == o); }
    };

    // const-callable: a zip piped into transform is walked through a const view (common/norm.hpp)
    iterator begin() const { return {std::begin(a), std::begin(b)}; }
    iterator end() const { return {std::end(a), std::end(b)}; }
};

// lvalue arguments are held by reference, rvalues by value
template <class A, class B>
zip_view<A, B> zip(A&& a, B&& b)
{
    return {std::forward<A>(a), std::forward<B>(b)};
}

} // namespace views
} // namespace ranges
