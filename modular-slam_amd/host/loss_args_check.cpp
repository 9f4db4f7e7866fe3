// loss_args_check.cpp — mslam::parseLoss (the harness's --loss argument) on accepted and refused texts.  A stand-alone
// program, built with the address and undefined-behaviour sanitizers (make loss_args_check): it exits 0 when every text is
// judged as listed and the refused ones leave kind and scale untouched.
#include "mslam_interfaces.hpp"

#include <cstdio>
#include <string>

int main()
{
    struct Case
    {
        const char* text;
        bool ok;
        int kind;
        double scale;
    };
    const Case cases[] = {
        {"huber:0.02", true, 1, 0.02},   {"cauchy:0.5", true, 2, 0.5},  {"huber:1e-3", true, 1, 1e-3}, {"cauchy:2", true, 2, 2.0},
        {"huber:", false, 0, 0},         {"huber", false, 0, 0},        {"", false, 0, 0},             {nullptr, false, 0, 0},
        {"huber:0", false, 0, 0},        {"huber:-1", false, 0, 0},     {"cauchy:inf", false, 0, 0},   {"cauchy:nan", false, 0, 0},
        {"huber:0.02x", false, 0, 0},    {"tukey:0.02", false, 0, 0},   {"Huber:0.02", false, 0, 0},   {"huber:1e999", false, 0, 0},
        {"cauchy: ", false, 0, 0},       {":0.02", false, 0, 0},        {"huber:0.02 ", false, 0, 0},  {"cauch", false, 0, 0},
    };
    int bad = 0;
    for(const Case& c : cases)
    {
        // the text in a heap block of its exact size: a read past its end is the sanitizer's to find
        std::string copy = c.text ? c.text : "";
        char* exact = c.text ? new char[copy.size() + 1] : nullptr;
        if(exact)
            std::memcpy(exact, copy.c_str(), copy.size() + 1);
        int kind = -7;
        double scale = -7.0;
        const bool ok = mslam::parseLoss(exact, kind, scale);
        const bool fine = ok == c.ok && (ok ? (kind == c.kind && scale == c.scale) : (kind == -7 && scale == -7.0));
        if(!fine)
        {
            std::fprintf(stderr, "parseLoss(\"%s\"): ok %d kind %d scale %g\n", c.text ? c.text : "(null)", ok ? 1 : 0, kind, scale);
            ++bad;
        }
        delete[] exact;
    }
    std::printf("loss_args_check: %zu texts, %d wrong\n", sizeof(cases) / sizeof(cases[0]), bad);
    return bad ? 1 : 0;
}
