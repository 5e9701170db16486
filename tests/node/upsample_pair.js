'use strict';
// Reduced-resolution rendering through the drop-in (INTEGRATION.md, "Rendering at reduced resolution"):
// a small NativeRenderer renders and denoises `frames` frames; a full-size one (scale times its
// size, same scene and default camera) runs only the G-buffer pass and Upsample(small).
//
// argv: JSON {sceneDir, width, height, scale, pipeline, frames, sigmaPlane, out}
// stdout: JSON {lo: [33 words], hi: [33 words], keys: [...Object.keys(addon)]}; the full-size
// renderer's ReadDenoised() goes to `${out}.hi.f32`, the small one's to `${out}.lo.f32`.
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
  for (let f = 0; f < req.frames; f++) {
    lo.Update();
    lo.Render();
  }
  lo.Denoise();
  hi.Update();
  hi.RunPass(PASS.GBUFFER);
  hi.Upsample(lo, req.sigmaPlane ? { sigmaPlane: req.sigmaPlane } : undefined);
  fs.writeFileSync(`${req.out}.hi.f32`, Buffer.from(hi.ReadDenoised().buffer));
  fs.writeFileSync(`${req.out}.lo.f32`, Buffer.from(lo.ReadDenoised().buffer));
  const res = { lo: Array.from(lo.Uniform), hi: Array.from(hi.Uniform), keys: Object.keys(addon) };
  hi.Destroy();
  lo.Destroy();
  process.stdout.write(JSON.stringify(res));
}
main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
