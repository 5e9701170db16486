'use strict';
// Temporal upsampling through the drop-in (INTEGRATION.md, "Rendering at reduced resolution"): a
// full-size NativeRenderer runs only its G-buffer pass; a small one renders one frame per phase
// through SetPhaseOf(full, scale, px, py), denoises it, and the full-size one integrates it with
// UpsampleTemporal(small, {px, py}).
//
// argv: JSON {sceneDir, width, height, scale, pipeline, phases: [[px, py], ...], alphaFill, out}
// stdout: JSON {hi: [33 words], lo: [[33 words] per phase], keys: [...Object.keys(addon)]}; the
// full-size renderer's ReadDenoised() goes to `${out}.hi.f32`, its ReadUpsampleHistory() to `${out}.hist.f32`.
const fs = require('fs');
const { NativeRenderer, PASS, addon } = require('../../pathtracerdemo_amd/js/NativeRenderer');
const { loadCompiledScene } = require('../../pathtracerdemo_amd/js/scene_io');

async function main() {
  const req = JSON.parse(process.argv[2]);
  const scene = loadCompiledScene(req.sceneDir);
  const make = (w, h) => new NativeRenderer(w, h, { pipeline: req.pipeline, device: 0 });
  const lo = make(req.width, req.height), hi = make(req.scale * req.width, req.scale * req.height);
  await lo.Initialize(scene);
  await hi.Initialize(scene);
  hi.Update();
  hi.RunPass(PASS.GBUFFER);
  const los = [];
  for (const [px, py] of req.phases) {
    lo.SetPhaseOf(hi, req.scale, px, py);
    lo.Render();
    lo.Denoise();
    const opts = { px, py };
    if (req.alphaFill !== undefined && req.alphaFill !== null) opts.alphaFill = req.alphaFill;
    hi.UpsampleTemporal(lo, opts);
    los.push(Array.from(lo.Uniform));
  }
  fs.writeFileSync(`${req.out}.hi.f32`, Buffer.from(hi.ReadDenoised().buffer));
  fs.writeFileSync(`${req.out}.hist.f32`, Buffer.from(hi.ReadUpsampleHistory().buffer));
  const res = { hi: Array.from(hi.Uniform), lo: los, keys: Object.keys(addon) };
  hi.Destroy();
  lo.Destroy();
  process.stdout.write(JSON.stringify(res));
}
main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
