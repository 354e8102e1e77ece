// `ezpz-amd`: the reference CLI's behaviour (ezpz-cli/src/main.rs) on top of the C ABI.
//   -f / --filepath <path|->   problem file, '-' for stdin            (main.rs:20-27, :225-238)
//   --show-points              print the final values                  (main.rs:33-35, :129-155)
//   -o / --image-path <png>    the solved sketch as a PNG file          (main.rs:28-32, visualize.rs:19-68): 1600 x 1600 pixels over
//                              the reference's span and palette, rasterised on the device (ezpz_sketch_image) and composed on the
//                              host (ezpz_sketch_compose); axes, mesh, caption and labels are not drawn
//   --cold                     extension: drop the topology cache before every timed solve
// Protocol (main.rs:81-103): parse, lower, solve once; lower again and solve 100 more times; report the mean
// over those 100 of the whole elapsed time.  Output lines follow main.rs:106-203.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ezpz_amd.h"
#include "png_write.hpp"

static const int NUM_ITERS_BENCHMARK = 100;  // main.rs:18

static const char* kKindNames[] = {
    "LineTangentToCircle", "CircleTangentToCircle", "Distance", "DistanceVar", "VerticalDistance", "HorizontalDistance",
    "Vertical", "Horizontal", "LinesAtAngle", "Fixed", "ScalarEqual", "PointsCoincident", "CircleRadius",
    "LinesEqualLength", "ArcRadius", "Arc", "Midpoint", "PointLineDistance", "VerticalPointLineDistance",
    "HorizontalPointLineDistance", "Symmetric", "PointArcCoincident", "ArcLength", "ArcAngle", "PointsAtAngle"};

static const char* warning_text(const EzpzWarning& w) {  // warnings.rs:62-83
    switch (w.content) {
    case EZPZ_WARN_DEGENERATE:
        return "This geometry is degenerate, meaning two points are so close together that they practically overlap. "
               "This is probably unintentional, you probably should place your initial guesses further apart or choose "
               "different constraints.";
    case EZPZ_WARN_SHOULD_BE_PARALLEL:
        return "Instead of constraining to this angle, constrain to Parallel";
    default:
        return "Instead of constraining to this angle, constraint to Perpendicular";
    }
}

static void print_problem_size(size_t num_vars, size_t num_eqs) {  // main.rs:194-203
    std::printf("Problem size: %zu rows, %zu vars\n", num_eqs, num_vars);
}

// The picture of the solved values x (visualize.rs:19-68; ezpz_amd/sketch_image.py: items_from_problem, fit_view, REFERENCE_LAYERS,
// restated): false when an entry fails.
static bool save_sketch_png(const EzpzProblem* parsed, const std::vector<double>& x, const std::string& path) {
    const uint32_t side = 1600;
    const double point_radius = 10.0, half_stroke = 1.5, padding = 1.0;
    const size_t np = ezpz_problem_num_labels(parsed, 0), nc = ezpz_problem_num_labels(parsed, 1), na = ezpz_problem_num_labels(parsed, 2);
    enum { POINTS, DISCS, CENTRES, ARCS, LINES, LAYERS };
    std::vector<EzpzDrawItem> items;
    auto add = [&](uint16_t kind, uint8_t layer, uint8_t flags, std::initializer_list<size_t> ids, double half_width) {
        EzpzDrawItem it;
        std::memset(&it, 0, sizeof it);
        it.kind = kind, it.layer = layer, it.flags = flags, it.half_width = half_width;
        int k = 0;
        for (size_t id : ids) it.ids[k++] = (uint32_t)id;
        items.push_back(it);
    };
    auto circle = [&](size_t i) { return 2 * np + 3 * i; };
    auto arc = [&](size_t i) { return 2 * np + 3 * nc + 6 * i; };  // a, b, centre
    for (size_t i = 0; i < np; ++i) add(EZPZ_DRAW_POINT, POINTS, 0, {2 * i, 2 * i + 1}, point_radius);
    for (size_t i = 0; i < nc; ++i) add(EZPZ_DRAW_POINT, CENTRES, 0, {circle(i), circle(i) + 1}, point_radius);
    for (size_t offset = 0; offset < 6; offset += 2)
        for (size_t i = 0; i < na; ++i) add(EZPZ_DRAW_POINT, ARCS, 0, {arc(i) + offset, arc(i) + offset + 1}, point_radius);
    for (size_t i = 0; i < nc; ++i) add(EZPZ_DRAW_CIRCLE, DISCS, EZPZ_DRAW_FILL, {circle(i), circle(i) + 1, circle(i) + 2}, 0.0);
    for (size_t i = 0; i < na; ++i) add(EZPZ_DRAW_ARC, ARCS, 0, {arc(i) + 4, arc(i) + 5, arc(i), arc(i) + 1, arc(i) + 2, arc(i) + 3}, half_stroke);
    for (size_t i = 0; i < ezpz_problem_num_lines(parsed); ++i) {
        size_t a = 0, b = 0;
        ezpz_problem_line(parsed, i, &a, &b);
        add(EZPZ_DRAW_SEGMENT, LINES, 0, {2 * a, 2 * a + 1, 2 * b, 2 * b + 1}, half_stroke);
    }
    // Bounds::new, visualize.rs:139-171: one span over both axes (a NaN is left out, as fmin and fmax leave it out)
    double lo_x = 0.0, hi_x = 0.0, lo_y = 0.0, hi_y = 0.0;
    bool any_x = false, any_y = false;
    auto take = [](double v, double& lo, double& hi, bool& any) {
        if (v != v) return;
        lo = any ? (v < lo ? v : lo) : v;
        hi = any ? (v > hi ? v : hi) : v;
        any = true;
    };
    for (const EzpzDrawItem& it : items) {
        if (it.kind == EZPZ_DRAW_CIRCLE) {
            for (double sign : {1.0, -1.0}) {
                take(x[it.ids[0]] + sign * x[it.ids[2]], lo_x, hi_x, any_x);
                take(x[it.ids[1]] + sign * x[it.ids[2]], lo_y, hi_y, any_y);
            }
        } else {
            const int pairs = it.kind == EZPZ_DRAW_POINT ? 1 : it.kind == EZPZ_DRAW_SEGMENT ? 2 : 3;
            for (int k = 0; k < pairs; ++k) take(x[it.ids[2 * k]], lo_x, hi_x, any_x), take(x[it.ids[2 * k + 1]], lo_y, hi_y, any_y);
        }
    }
    const double lo = lo_x - padding < lo_y - padding ? lo_x - padding : lo_y - padding;
    const double hi = hi_x + padding > hi_y + padding ? hi_x + padding : hi_y + padding;
    EzpzImageView view;
    view.x_min = lo, view.y_min = lo, view.scale = (double)side / (hi - lo), view.width = side, view.height = side;
    std::vector<uint32_t> counts((size_t)LAYERS * side * side);
    EzpzImageInfo info;
    int rc = ezpz_sketch_image(x.data(), nullptr, 1, x.size(), items.data(), items.size(), &view, LAYERS, 0, counts.data(), &info);
    if (rc != EZPZ_OK) {
        std::fprintf(stderr, "Error: could not draw the sketch: %s\n", ezpz_error_string(rc));
        return false;
    }
    // visualize.rs:7-10; the discs at the reference's mix(0.3)
    static const EzpzComposeLayer layers[LAYERS] = {{{0x58, 0x50, 0x8d}, 255, 0, 1}, {{0xbc, 0x50, 0x90}, 77, 0, 1}, {{0xbc, 0x50, 0x90}, 255, 0, 1},
                                                    {{0xff, 0x63, 0x61}, 255, 0, 1}, {{0xff, 0xa6, 0x00}, 255, 0, 1}};
    static const uint8_t white[3] = {255, 255, 255};
    std::vector<uint8_t> rgb((size_t)side * side * 3), flipped(rgb.size());
    if (ezpz_sketch_compose(counts.data(), &view, LAYERS, layers, white, rgb.data()) != EZPZ_OK) return false;
    for (uint32_t y = 0; y < side; ++y)  // row 0 is y_min: the bottom of the picture
        std::memcpy(&flipped[(size_t)y * side * 3], &rgb[(size_t)(side - 1 - y) * side * 3], (size_t)side * 3);
    if (!ezpz::png::write_file(path.c_str(), flipped.data(), side, side)) {
        std::fprintf(stderr, "Error: could not write %s\n", path.c_str());
        return false;
    }
    std::printf("Plot saved to %s\n", path.c_str());  // visualize.rs:66
    return true;
}

int main(int argc, char** argv) {
    std::string filepath, image_path;
    bool show_points = false, cold = false;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if ((a == "-f" || a == "--filepath") && i + 1 < argc)
            filepath = argv[++i];
        else if (a.rfind("--filepath=", 0) == 0)
            filepath = a.substr(11);
        else if (a == "--show-points")
            show_points = true;
        else if (a == "--cold")
            cold = true;
        else if ((a == "-o" || a == "--image-path") && i + 1 < argc)
            image_path = argv[++i];
        else if (a.rfind("--image-path=", 0) == 0)
            image_path = a.substr(13);
        else if (a == "-h" || a == "--help") {
            std::printf("Usage: ezpz-amd --filepath <FILEPATH> [--show-points] [--image-path <PNG>] [--cold]\n"
                        "  -o, --image-path <PNG>  write the solved sketch as a 1600 x 1600 PNG file\n");
            return 0;
        } else {
            std::fprintf(stderr, "error: unexpected argument '%s'\n", a.c_str());
            return 2;
        }
    }
    if (filepath.empty()) {
        std::fprintf(stderr, "error: the following required arguments were not provided:\n  --filepath <FILEPATH>\n");
        return 2;
    }
    std::string text;
    if (filepath == "-") {
        std::stringstream ss;
        ss << std::cin.rdbuf();
        text = ss.str();
    } else {
        std::ifstream f(filepath);
        if (!f) {
            std::fprintf(stderr, "Error: No such file or directory (os error 2)\n");
            return 1;
        }
        std::stringstream ss;
        ss << f.rdbuf();
        text = ss.str();
    }
    char err[512] = {0};
    EzpzProblem* parsed = nullptr;
    auto now = std::chrono::steady_clock::now();
    int rc = ezpz_problem_parse(text.data(), text.size(), &parsed, err, sizeof(err));
    if (rc != EZPZ_OK) {
        std::fprintf(stderr, "Error: %s\n", err[0] ? err : ezpz_error_string(rc));
        return 1;
    }
    const size_t n_cs = ezpz_problem_num_constraints(parsed), n = ezpz_problem_num_vars(parsed);
    const EzpzConstraint* cs = ezpz_problem_constraints(parsed);
    const double* guesses = ezpz_problem_guesses(parsed);
    std::vector<uint32_t> ids(n);
    for (size_t i = 0; i < n; ++i) ids[i] = (uint32_t)i;
    std::vector<double> x(n ? n : 1);
    std::vector<uint64_t> unsat(n_cs + 1);
    std::vector<EzpzWarning> warns(4096);
    EzpzConfig cfg;
    ezpz_default_config(&cfg);
    EzpzOutcome out;
    rc = ezpz_solve(cs, n_cs, ids.data(), guesses, n, &cfg, x.data(), unsat.data(), warns.data(), warns.size(), &out);
    size_t nw = out.n_warnings < warns.size() ? (size_t)out.n_warnings : warns.size();
    auto print_warnings = [&]() {  // main.rs:172-180
        if (nw) {
            std::printf("Warnings:\n");
            for (size_t i = 0; i < nw; ++i) std::printf("\t%s\n", warning_text(warns[i]));
        }
    };
    if (rc != EZPZ_OK) {  // print_failure_output, main.rs:205-223
        print_warnings();
        print_problem_size(out.num_vars, out.num_eqs);
        std::fprintf(stderr, "Could not solve system: %s\n", ezpz_error_string(rc));
        if (out.num_eqs > out.num_vars)
            std::fprintf(stderr, "Your system might be overconstrained. Try removing constraints.\n");
        else
            std::fprintf(stderr, "You might have contradictory constraints.\n");
        return 1;
    }
    // It succeeded. Benchmark its perf (main.rs:93-100): a second lowering, then 100 solves.
    EzpzProblem* again = nullptr;
    ezpz_problem_parse(text.data(), text.size(), &again, err, sizeof(err));
    std::vector<double> x2(n ? n : 1);
    std::vector<uint64_t> unsat2(n_cs + 1);
    EzpzOutcome o2;
    auto loop_start = std::chrono::steady_clock::now();
    for (int i = 0; i < NUM_ITERS_BENCHMARK; ++i) {
        if (cold) ezpz_cache_clear();
        ezpz_solve(ezpz_problem_constraints(again), n_cs, ids.data(), ezpz_problem_guesses(again), n, &cfg, x2.data(),
                   unsat2.data(), nullptr, 0, &o2);
    }
    auto loop_end = std::chrono::steady_clock::now();
    auto elapsed = loop_end - now;
    const double steady_us = std::chrono::duration<double, std::micro>(loop_end - loop_start).count() / NUM_ITERS_BENCHMARK;
    const double first_ms = std::chrono::duration<double, std::milli>(loop_start - now).count();
    const long long micros =
        std::chrono::duration_cast<std::chrono::microseconds>(elapsed).count() / NUM_ITERS_BENCHMARK;

    print_warnings();
    if (out.n_unsatisfied) {  // main.rs:182-192
        std::printf("Not all constraints were satisfied:\n");
        for (uint64_t i = 0; i < out.n_unsatisfied; ++i) {
            const EzpzConstraint& c = cs[unsat[i]];
            std::printf("\t%llu: %s\n", (unsigned long long)unsat[i], c.kind < 25 ? kKindNames[c.kind] : "?");
        }
    }
    print_problem_size(out.num_vars, out.num_eqs);
    std::printf("Iterations needed: %llu\n", (unsigned long long)out.iterations);
    std::printf("Solved up to priority: %u\n", out.priority_solved);
    if (!out.converged) std::printf("Error: solver did not converge!\n");
    std::printf("Solved in %lldμs (mean over %d iterations)\n", micros, NUM_ITERS_BENCHMARK);
    std::printf("i.e. %lld solves per second\n", micros > 0 ? 1000000LL / micros : 0LL);
    // extension: the reference's mean includes the first solve, which here carries the one-time GPU context and
    // code-object load; the loop alone is the per-solve cost a long-lived process sees.
    std::printf("Steady state: %.1fμs per solve, i.e. %.0f solves per second (first solve incl. device init: %.1f ms)\n",
                steady_us, steady_us > 0 ? 1e6 / steady_us : 0.0, first_ms);
    if (show_points) {  // main.rs:129-155, label order executor.rs:525-566
        const size_t np = ezpz_problem_num_labels(parsed, 0), nc = ezpz_problem_num_labels(parsed, 1),
                     na = ezpz_problem_num_labels(parsed, 2);
        std::printf("Points:\n");
        for (size_t i = 0; i < np; ++i)
            std::printf("\t%s: (%.2f, %.2f)\n", ezpz_problem_label(parsed, 0, i), x[2 * i], x[2 * i + 1]);
        if (nc) {
            std::printf("Circles:\n");
            for (size_t i = 0; i < nc; ++i) {
                size_t s = 2 * np + 3 * i;
                std::printf("\t%s: center = (%.2f, %.2f), radius = %.2f\n", ezpz_problem_label(parsed, 1, i), x[s], x[s + 1],
                            x[s + 2]);
            }
        }
        if (na) {
            std::printf("Arcs:\n");
            for (size_t i = 0; i < na; ++i) {
                size_t s = 2 * np + 3 * nc + 6 * i;
                std::printf("\t%s: center = (%.2f, %.2f), a = (%.2f, %.2f), b = (%.2f, %.2f)\n",
                            ezpz_problem_label(parsed, 2, i), x[s + 4], x[s + 5], x[s], x[s + 1], x[s + 2], x[s + 3]);
            }
        }
    }
    bool drawn = true;
    if (!image_path.empty()) {
        x.resize(n);
        drawn = save_sketch_png(parsed, x, image_path);
    }
    ezpz_problem_destroy(parsed);
    ezpz_problem_destroy(again);
    return drawn ? 0 : 1;
}
